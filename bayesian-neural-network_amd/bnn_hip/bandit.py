"""F5: the mushroom contextual bandit of the reference (reinforcement_learning/base_bandit.py, bandits.py:17-54) with the
whole loop on the device.

One reference step (base_bandit.py:75-99) decides with 2 x n_samples batch-1 forwards that each end in `.item()`, appends
to Python lists, rebuilds up to buffer_size rows from them through a numpy permutation and then runs up to num_batches
dependent training steps, each launch-bound.  Here a step is

    decision   bnn_bandit_rows -> the network's forward of the A rows -> bnn_bandit_act     (one hipGraph / recorded calls)
    replay     bnn_bandit_replay: pool, shuffle (bitonic sort in LDS), gather into the minibatch slab (a second graph)
    training   nb(t) replays of train.GraphedTrainStep on slab[j] with beta_j, then scheduler.step()

and nothing is read back: the step number, the replay ring, the regrets and the counts live on the device, and the host
knows nb(t) from t alone (`n_batches`).  Semantics are include/bnn_hip.h F5's; the random decisions (the epsilon-greedy
coin, the reward coin, a drawn context, the permutation) come from the bandit's own Philox stream (word 3 = 1), the
network's epsilon from the usual one (word 3 = 0), so the two never share a counter.

The MUSHROOM table reproduces base_bandit.py:26-35 BY LABEL VALUE, as the reference reads its labels: read_data_rl's
LabelEncoder maps 'e' -> 0, 'p' -> 1 and the reference calls that value `edible`, so label 1 earns +5 for eating and label
0 earns +5 or -35 (probability 1/2 each); rejecting earns 0 and the oracle is 5 * label.  Kept as the reference has it.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from . import ops
from .capture import capture_on_side_stream
from .ops import BnnHipError
from .optim import FusedAdam
from .runtime import state


class RewardTable(NamedTuple):
    """rewards[k][a] = (hi, lo, thr): the reward of action a on label k is hi when the step's coin u > thr, else lo;
    oracle[k] is the best expected reward of label k (the regret's reference)."""
    rewards: tuple
    oracle: tuple


# base_bandit.py:26-35 by label value (module docstring): action 0 = eat, 1 = reject
MUSHROOM = RewardTable(rewards=(((5.0, -35.0, 0.5), (0.0, 0.0, 0.5)),      # label 0: eat 5 if rand > 0.5 else -35
                                ((5.0, 5.0, 0.5), (0.0, 0.0, 0.5))),       # label 1: eat 5
                       oracle=(0.0, 5.0))


# ---------------------------------------------------------------------------------------------------- host schedule
def pool_size(l: int, batch_size: int, buffer_size: int) -> int:
    """Entries of the replay pool after l appends (base_bandit.py:77-84)."""
    if l <= 0:
        return 0
    if l <= batch_size:
        return batch_size
    if l < buffer_size:
        return l // batch_size * batch_size
    return buffer_size


def n_batches(t: int, batch_size: int, buffer_size: int) -> int:
    """Training minibatches of bandit step t (0-based): a function of t alone, so the host never reads it back."""
    return pool_size(t + 1, batch_size, buffer_size) // batch_size


def pool_entries(l: int, batch_size: int, buffer_size: int) -> np.ndarray:
    """Buffer entries (0-based append order) at the pool positions, before the shuffle."""
    P = pool_size(l, batch_size, buffer_size)
    p = np.arange(P, dtype=np.int64)
    if l <= batch_size:
        m = batch_size // l + 1
        return (m * l - batch_size + p) % l
    return l - P + p


def beta(j: int, num_batches: int) -> float:
    """KL weight of minibatch j (bandits.py:44); num_batches is the configured value, not nb."""
    return 2 ** (num_batches - (j + 1)) / (2 ** num_batches - 1)


# ---------------------------------------------------------------------------------------------------- the agent
class BNNBandit:
    """BNN_Bandit (bandits.py:17-54) on the device.  `bandit_params` takes the keys of main.py:76-87 (+ n_samples, epsilon);
    `x` [N, d] contexts, `y` [N] labels in [0, K).

    policy="mean": the reference's rule -- every one of the n_samples outputs is the deterministic forward (net(x) in eval
    mode, base_bandit.py:44-46), so n_samples only scales the sum.  policy="thompson": output s is the forward under posterior
    draw s (one weight draw for all A action rows of the decision, a fresh global MC-sample index per draw, taken from the
    counter the training step shares).  A local-reparameterisation network draws activation noise per row, not a function,
    so it serves policy="mean" only.

    Mirrors bandits.py:23-37: `net` (networks.BayesianNetwork, local_reparam filled in), `optimiser` (FusedAdam,
    capturable), `scheduler` (StepLR(step_size=5000, gamma=0.5), stepped by update()).  `cumulative_regrets`, `tp`, `tn`,
    `fp`, `fn`, `counts` read device state: EACH READ SYNCHRONISES with the device once.  update() never does.
    `capture`: True (hipGraphs), "calls" (recorded launch lists) or False (eager launches)."""

    def __init__(self, label, bandit_params, x, y, *, policy: str = "thompson", rewards: RewardTable = MUSHROOM,
                 seed: Optional[int] = None, max_steps: int = 50000, local_reparam: bool = False, capture=True):
        import networks
        from .engine import effective_math
        from .train import GraphedTrainStep
        if state.shard_samples:
            raise BnnHipError("BNNBandit: sample sharding is not supported (one device runs the whole loop)")
        if policy not in ("mean", "thompson"):
            raise BnnHipError(f"BNNBandit: policy must be 'mean' or 'thompson', got {policy!r}")
        if policy == "thompson" and local_reparam:
            raise BnnHipError("BNNBandit: Thompson sampling needs weight draws; a local-reparameterisation network draws "
                              "activation noise per row -- use policy='mean'")
        p = bandit_params
        self.label = label
        self.n_samples, self.buffer_size = int(p["n_samples"]), int(p["buffer_size"])
        self.batch_size, self.num_batches = int(p["batch_size"]), int(p["num_batches"])
        self.lr, self.epsilon = float(p["lr"]), float(p["epsilon"])
        self.policy, self.max_steps = policy, int(max_steps)
        if self.buffer_size % self.batch_size:
            raise BnnHipError("BNNBandit: buffer_size must be a multiple of batch_size (the reference's last minibatch is short)")
        if not 0 < self.buffer_size <= L.BANDIT_MAX_BUFFER:
            raise BnnHipError(f"BNNBandit: buffer_size must lie in [1, {L.BANDIT_MAX_BUFFER}]")
        if self.n_samples < 1 or self.max_steps < 1:
            raise BnnHipError("BNNBandit: n_samples and max_steps must be positive")
        dev = torch.device("cuda", torch.cuda.current_device())
        self.x = torch.as_tensor(np.asarray(x), dtype=torch.float32).to(dev).contiguous()
        yh = np.asarray(y).astype(np.int64)
        tab = np.asarray(rewards.rewards, dtype=np.float32)
        if tab.ndim != 3 or tab.shape[2] != 3 or tab.shape[1] < 2 or len(rewards.oracle) != tab.shape[0]:
            raise BnnHipError("BNNBandit: rewards must be [K][A][(hi, lo, thr)] with A >= 2 and K oracle values")
        self.K, self.A = tab.shape[0], tab.shape[1]
        if self.x.dim() != 2 or yh.shape != (self.x.shape[0],) or yh.min() < 0 or yh.max() >= self.K:
            raise BnnHipError("BNNBandit: x must be [N, d] and y [N] labels in [0, K)")
        self.N, self.d = self.x.shape
        self.y = torch.from_numpy(yh).to(dev)
        self.table = torch.from_numpy(tab).to(dev)
        self.oracle = torch.tensor(rewards.oracle, dtype=torch.float32, device=dev)
        self.seed = state.seed if seed is None else int(seed)

        # bandits.py:23-37
        model_params = {
            'input_shape': self.d + self.A, 'classes': 1, 'batch_size': self.batch_size,
            'hidden_units': p['hidden_units'], 'mode': p['mode'], 'mixture_prior': p['mixture_prior'],
            'mu_init': p['mu_init'], 'rho_init': p['rho_init'], 'prior_init': p['prior_init'],
            'local_reparam': bool(local_reparam),
        }
        if model_params['mode'] != 'regression':
            raise BnnHipError("BNNBandit: the bandit's network regresses the reward (mode='regression')")
        self.net = networks.BayesianNetwork(model_params).to(dev)
        self.optimiser = FusedAdam(self.net.parameters(), lr=self.lr, capturable=True)
        self.scheduler = torch.optim.lr_scheduler.StepLR(self.optimiser, step_size=5000, gamma=0.5)

        # device state
        i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
        T, B, W = self.max_steps, self.buffer_size, self.d + self.A
        self.step_word = torch.zeros(1, **i32)
        self.cur_index = torch.zeros(1, **i32)
        self.indices = torch.full((T,), -1, dtype=torch.int64, device=dev)         # -1: draw the context on the device
        self.actions = torch.zeros(T, dtype=torch.int64, device=dev)
        self.rewards = torch.zeros(T, **f32)
        self.regrets = torch.zeros(T + 1, dtype=torch.float64, device=dev)
        self._counts = torch.zeros((self.K, self.A), dtype=torch.int64, device=dev)
        self.ring_index, self.ring_action, self.ring_reward = torch.zeros(B, **i32), torch.zeros(B, **i32), torch.zeros(B, **f32)
        self.perm = torch.zeros(B, **i32)
        self.nb_slab = B // self.batch_size
        self.slab = torch.zeros((self.nb_slab, self.batch_size, W), **f32)
        self.targets = torch.zeros((self.nb_slab, self.batch_size, 1), **f32)
        self.rows = torch.zeros((self.A, W), **f32)
        self.t = 0
        self.loss_info = None

        self.train = GraphedTrainStep(self.net, self.optimiser, self.slab[0], self.targets[0], self.n_samples)

        # the decision forward: S draws (thompson) or the one deterministic forward (mean) of the A rows
        self.math = effective_math(bool(local_reparam))
        hid = torch.bfloat16 if (self.math == L.MATH_BF16 and not local_reparam) else torch.float32
        self.specs = self.net._specs()
        n = self.n_samples if policy == "thompson" else 1
        self.dec_samples = n
        self.h = [torch.empty((n, self.A, sp.in_out[1]), dtype=torch.float32 if i == len(self.specs) - 1 else hid, device=dev)
                  for i, sp in enumerate(self.specs)]
        self.act_args = ops.bandit_act_args(
            x=self.x, labels=self.y, rewards=self.table, oracle=self.oracle, outputs=self.h[-1], n_samples=self.n_samples,
            output_sample_stride=self.A if policy == "thompson" else 0, step=self.step_word, cur_index=self.cur_index,
            rows=self.rows, actions=self.actions, reward_out=self.rewards, regrets=self.regrets, counts=self._counts,
            ring_index=self.ring_index, ring_action=self.ring_action, ring_reward=self.ring_reward, epsilon=self.epsilon,
            seed=self.seed, indices=self.indices, sample_counter=self.train.counter if policy == "thompson" else None,
            sample_counter_inc=n if policy == "thompson" else 0)
        self.replay_args = ops.bandit_replay_args(
            x=self.x, step=self.step_word, ring_index=self.ring_index, ring_action=self.ring_action, ring_reward=self.ring_reward,
            workspace=self.perm, slab=self.slab, targets=self.targets, batch_size=self.batch_size, n_actions=self.A, seed=self.seed)

        # warm-up (validates every argument block eagerly; "calls" records it), then the state words are reset
        self.capture = capture
        self.calls_decide = self.calls_replay = None
        self.g_decide = self.g_replay = None
        self.train._shared.sync()
        mirror = self.train._shared["mirror"]
        if capture == "calls":
            with L.recording() as calls:
                self._decide()
            self.calls_decide = list(calls)
            with L.recording() as calls:
                self._replay()
            self.calls_replay = list(calls)
        else:
            self._decide()
            self._replay()
        torch.cuda.synchronize()
        self._reset_words(mirror)
        if capture is True:
            self.g_decide, self.g_replay = capture_on_side_stream(self._decide, self._replay)
        elif capture not in ("calls", False):
            raise BnnHipError(f"BNNBandit: capture must be True, 'calls' or False, got {capture!r}")
        torch.cuda.synchronize()

    def _reset_words(self, mirror: int):
        self.step_word.zero_()
        self._counts.zero_()
        self.regrets.zero_()
        self.train._shared.set(mirror)

    def _decide(self):
        """bnn_bandit_rows -> forward of the A rows -> bnn_bandit_act, on the current stream."""
        ops.bandit_rows(self.act_args)
        thompson = self.policy == "thompson"
        eps_mode = L.EPS_PHILOX if thompson else L.EPS_ZERO
        h = self.rows
        for i, sp in enumerate(self.specs):
            m = sp.m
            pd = (m.weight_mu.detach(), m.weight_rho.detach(), m.bias_mu.detach(), m.bias_rho.detach())
            kw = dict(n_samples=self.dec_samples, math_mode=self.math, relu=sp.relu, y_dtype=self.h[i].dtype, eps_mode=eps_mode,
                      seed=state.seed, layer_id=sp.layer_id, sample_offset=self.train.base if thompson else 0,
                      sample_counter=self.train.counter if thompson else None, form=state.form, out=self.h[i])
            if sp.lr:
                ops.lr_linear_fwd(h, *pd, sigma_p=m._prior_spec.sigma_p, want_kl=False, **kw)
            else:
                ops.bbb_linear_fwd(h, *pd, prior=m._prior_spec, want_stats=False, **kw)
            h = self.h[i]
        ops.bandit_act(self.act_args)

    def _replay(self):
        ops.bandit_replay(self.replay_args)

    @staticmethod
    def _run_calls(calls):
        for fn, args, name in calls:
            rc = fn(*args)
            if rc:
                L.check(rc, name)

    def _step(self):
        if state.shard_samples:
            raise BnnHipError("BNNBandit: sample sharding is not supported")
        t = self.t
        thompson = self.policy == "thompson"
        counter = self.train._shared
        if thompson:
            counter.sync()
        if self.g_decide is not None:
            self.g_decide.replay()
            if thompson:
                counter.advance(self.dec_samples)
            self.g_replay.replay()
        elif self.calls_decide is not None:
            self._run_calls(self.calls_decide)
            if thompson:
                counter.advance(self.dec_samples)
            self._run_calls(self.calls_replay)
        else:
            self._decide()
            if thompson:
                counter.advance(self.dec_samples)
            self._replay()
        for j in range(n_batches(t, self.batch_size, self.buffer_size)):
            self.loss_info = self.train.step(self.slab[j], self.targets[j], beta(j, self.num_batches))
        self.scheduler.step()
        self.t = t + 1

    def update(self, mushroom: Optional[int] = None):
        """One bandit step (base_bandit.py:75-84 + the training of bandits.py:43-51 + main.py:103's scheduler.step()) on
        context `mushroom`, or on a context drawn on the device when None.  Does not synchronise with the host."""
        if self.t >= self.max_steps:
            raise BnnHipError(f"BNNBandit: max_steps={self.max_steps} reached")
        if mushroom is not None:
            i = int(mushroom)
            if not 0 <= i < self.N:
                raise BnnHipError(f"BNNBandit: context index {i} outside [0, {self.N})")
            self.indices[self.t].fill_(i)
        self._step()

    def run(self, indices: Sequence[int]):
        """update(i) for every i of `indices`, the sequence uploaded once."""
        idx = np.asarray(indices, dtype=np.int64).reshape(-1)
        if self.t + idx.size > self.max_steps:
            raise BnnHipError(f"BNNBandit: {idx.size} steps from step {self.t} pass max_steps={self.max_steps}")
        if idx.size and (idx.min() < 0 or idx.max() >= self.N):
            raise BnnHipError(f"BNNBandit: context indices must lie in [0, {self.N})")
        self.indices[self.t:self.t + idx.size].copy_(torch.from_numpy(idx))
        for _ in range(idx.size):
            self._step()

    # ---- reads (each one synchronises)
    @property
    def cumulative_regrets(self) -> list:
        """[0, r_1, ..., r_t] as base_bandit.py:20, :99 keep it (fp64)."""
        return self.regrets[:self.t + 1].tolist()

    @property
    def counts(self) -> np.ndarray:
        """counts[label, action] (int64)."""
        return self._counts.cpu().numpy()

    @property
    def tp(self) -> int:
        return int(self._counts[1, 0].item())

    @property
    def fn(self) -> int:
        return int(self._counts[1, 1].item())

    @property
    def fp(self) -> int:
        return int(self._counts[0, 0].item())

    @property
    def tn(self) -> int:
        return int(self._counts[0, 1].item())

    def history(self):
        """(actions [t] int64, rewards [t] fp32) of the steps taken, as numpy arrays."""
        return self.actions[:self.t].cpu().numpy(), self.rewards[:self.t].cpu().numpy()


# ---------------------------------------------------------------------------------------------------- F6 greedy agents
class GreedyBanditGroup:
    """G independent Greedy_Bandit agents (bandits.py:59-85: an MLP in-(hidden)-(hidden)-1 trained with Adam on
    mse_loss(net(x).squeeze(), y, reduction='sum'), epsilon-greedy decisions) advanced together on the device.  One update
    of the whole group is six launches whatever G (include/bnn_hip.h F6), one workgroup per agent in each:

        bnn_bandit_rows_group -> bnn_mlp_group_fwd -> bnn_bandit_act_group -> bnn_bandit_replay_group (2)
        -> bnn_mlp_group_train (all nb minibatch steps of every agent)

    captured as one hipGraph (`capture=True`) or launched eagerly (`capture=False`); the host never reads anything back.

    G = len(epsilons).  Agent g builds networks.MLP exactly as Greedy_Bandit.init_net does, in order under torch's RNG, with
    a capturable FusedAdam(lr=bandit_params['lr']) and StepLR(step_size=5000, gamma=0.5), and has its own bandit Philox
    stream (seeds[g]; by default the global seed + g), ring, regrets, counts, actions and rewards.  update(mushroom) and
    run(indices) give every agent the same context, as main.py does; update() without an index lets each agent draw its
    context from its own stream.  `group[g]` is agent g's view (the BNNBandit read surface); every read synchronises."""

    def __init__(self, label, bandit_params, x, y, *, epsilons, seeds=None, rewards: RewardTable = MUSHROOM,
                 max_steps: int = 50000, capture: bool = True):
        import networks
        p = bandit_params
        if state.shard_samples:
            raise BnnHipError("GreedyBanditGroup: sample sharding is not supported (one device runs the whole loop)")
        if p["mode"] != "regression":
            raise BnnHipError("GreedyBanditGroup: the bandit's network regresses the reward (mode='regression')")
        self.label = label
        self.buffer_size, self.batch_size = int(p["buffer_size"]), int(p["batch_size"])
        self.num_batches, self.lr, self.hidden = int(p["num_batches"]), float(p["lr"]), int(p["hidden_units"])
        self.max_steps = int(max_steps)
        if self.batch_size < 1 or self.buffer_size % self.batch_size:
            raise BnnHipError("GreedyBanditGroup: buffer_size must be a multiple of batch_size (the reference's last "
                              "minibatch is short)")
        eps = [float(e) for e in epsilons]
        if not eps or any(not 0.0 <= e <= 1.0 for e in eps):                    # NaN fails the comparison
            raise BnnHipError(f"GreedyBanditGroup: epsilons must be a non-empty list of values in [0, 1], got {epsilons!r}")
        self.G = len(eps)
        if seeds is not None and len(seeds) != self.G:
            raise BnnHipError(f"GreedyBanditGroup: {len(seeds)} seeds for {self.G} epsilons")
        tab = np.asarray(rewards.rewards, dtype=np.float32)
        if tab.ndim != 3 or tab.shape[2] != 3 or tab.shape[1] < 2 or len(rewards.oracle) != tab.shape[0]:
            raise BnnHipError("GreedyBanditGroup: rewards must be [K][A][(hi, lo, thr)] with A >= 2 and K oracle values")
        self.K, self.A = tab.shape[0], tab.shape[1]
        xh, yh = np.asarray(x, dtype=np.float32), np.asarray(y).astype(np.int64)
        if xh.ndim != 2 or yh.shape != (xh.shape[0],) or yh.min() < 0 or yh.max() >= self.K:
            raise BnnHipError("GreedyBanditGroup: x must be [N, d] and y [N] labels in [0, K)")
        self.N, self.d = xh.shape
        W = self.d + self.A
        nbm = self.buffer_size // self.batch_size
        if (W > L.MLP_GROUP_MAX_IN or not 1 <= self.hidden <= L.MLP_GROUP_MAX_HIDDEN or self.batch_size > L.MLP_GROUP_MAX_BATCH
                or nbm > L.MLP_GROUP_MAX_BATCHES or self.A > min(L.BANDIT_MAX_ACTIONS, L.MLP_GROUP_MAX_BATCH)
                or self.buffer_size > L.BANDIT_MAX_BUFFER or self.G > L.MLP_GROUP_MAX_AGENTS or self.max_steps < 1):
            raise BnnHipError(f"GreedyBanditGroup: beyond the kernels' limits (input {W} <= {L.MLP_GROUP_MAX_IN}, hidden <= "
                              f"{L.MLP_GROUP_MAX_HIDDEN}, batch <= {L.MLP_GROUP_MAX_BATCH}, buffer / batch <= "
                              f"{L.MLP_GROUP_MAX_BATCHES}, buffer <= {L.BANDIT_MAX_BUFFER}, agents <= {L.MLP_GROUP_MAX_AGENTS})")
        self.epsilons = eps
        self.seeds = [state.seed + g if seeds is None else int(seeds[g]) for g in range(self.G)]

        dev = torch.device("cuda", torch.cuda.current_device())
        self.x = torch.from_numpy(xh).to(dev).contiguous()
        self.y = torch.from_numpy(yh).to(dev)
        self.table = torch.from_numpy(tab).to(dev)
        self.oracle = torch.tensor(rewards.oracle, dtype=torch.float32, device=dev)

        # bandits.py:64-74, agent by agent
        model_params = {'input_shape': W, 'classes': 1, 'batch_size': self.batch_size, 'hidden_units': self.hidden,
                        'mode': p['mode']}
        self.nets, self.optimisers, self.schedulers = [], [], []
        for g in range(self.G):
            net = networks.MLP(model_params).to(dev)
            opt = FusedAdam(net.parameters(), lr=self.lr, capturable=True)
            self.nets.append(net)
            self.optimisers.append(opt)
            self.schedulers.append(torch.optim.lr_scheduler.StepLR(opt, step_size=5000, gamma=0.5))

        # device state, [G, ...] with one contiguous row per agent
        G, T, B = self.G, self.max_steps, self.buffer_size
        i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
        self.step_word = torch.zeros((G, 1), **i32)
        self.cur_index = torch.zeros((G, 1), **i32)
        self.indices = torch.full((T,), -1, dtype=torch.int64, device=dev)       # shared: -1 = each agent draws its own
        self.actions = torch.zeros((G, T), dtype=torch.int64, device=dev)
        self.rewards = torch.zeros((G, T), **f32)
        self.regrets = torch.zeros((G, T + 1), dtype=torch.float64, device=dev)
        self._counts = torch.zeros((G, self.K, self.A), dtype=torch.int64, device=dev)
        self.ring_index, self.ring_action, self.ring_reward = torch.zeros((G, B), **i32), torch.zeros((G, B), **i32), \
            torch.zeros((G, B), **f32)
        self.perm = torch.zeros((G, B), **i32)
        self.nb_slab = nbm
        self.slab = torch.zeros((G, nbm, self.batch_size, W), **f32)
        self.targets = torch.zeros((G, nbm, self.batch_size), **f32)
        self.n_batches_word = torch.zeros((G, 1), **i32)
        self.loss = torch.zeros((G, 1), **f32)
        self.rows = torch.zeros((G, self.A, W), **f32)
        self.outputs = torch.zeros((G, self.A), **f32)
        self.t = 0

        act, rep, mlp = [], [], []
        for g in range(G):
            act.append(ops.bandit_act_args(
                x=self.x, labels=self.y, rewards=self.table, oracle=self.oracle, outputs=self.outputs[g], n_samples=1,
                output_sample_stride=0, step=self.step_word[g], cur_index=self.cur_index[g], rows=self.rows[g],
                actions=self.actions[g], reward_out=self.rewards[g], regrets=self.regrets[g], counts=self._counts[g],
                ring_index=self.ring_index[g], ring_action=self.ring_action[g], ring_reward=self.ring_reward[g],
                epsilon=eps[g], seed=self.seeds[g], indices=self.indices))
            rep.append(ops.bandit_replay_args(
                x=self.x, step=self.step_word[g], ring_index=self.ring_index[g], ring_action=self.ring_action[g],
                ring_reward=self.ring_reward[g], workspace=self.perm[g], slab=self.slab[g], targets=self.targets[g],
                batch_size=self.batch_size, n_actions=self.A, seed=self.seeds[g], n_batches=self.n_batches_word[g]))
            opt = self.optimisers[g]
            params = [t.detach() for t in self.nets[g].parameters()]              # w1 b1 w2 b2 w3 b3
            for q in self.nets[g].parameters():                                   # Adam's state, as its first step makes it
                st = opt.state[q]
                st["step"] = 0
                st["exp_avg"] = torch.zeros_like(q, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(q, memory_format=torch.preserve_format)
            step_dev, lr_dev, _, _ = opt._group_dev(0, opt.param_groups[0], dev)
            qs = list(self.nets[g].parameters())
            mlp.append(ops.mlp_group_agent(
                params=params, exp_avg=[opt.state[q]["exp_avg"] for q in qs], exp_avg_sq=[opt.state[q]["exp_avg_sq"] for q in qs],
                step=step_dev, lr=lr_dev, slab=self.slab[g], targets=self.targets[g], n_batches=self.n_batches_word[g],
                loss=self.loss[g], rows=self.rows[g], outputs=self.outputs[g]))
        grp = self.optimisers[0].param_groups[0]
        self.g_act = ops.bandit_group_args(act, dev)
        self.g_replay = ops.bandit_group_args(rep, dev)
        shape = dict(in_features=W, hidden=self.hidden, device=dev, betas=grp["betas"], eps=grp["eps"],
                     weight_decay=grp["weight_decay"])
        self.g_fwd = ops.mlp_group_args(mlp, n_rows=self.A, **shape)
        self.g_train = ops.mlp_group_args(mlp, batch=self.batch_size, max_batches=nbm, **shape)

        # warm-up: every launch once, eagerly (this validates every block); the training launch with nb = 0 touches nothing.
        # Then the words the warm-up moved are reset, and the update is captured.
        self.capture = bool(capture)
        self.graph = None
        self._enqueue(train=False)
        self.n_batches_word.zero_()
        ops.mlp_group_train(self.g_train)
        torch.cuda.synchronize()
        self.step_word.zero_()
        self._counts.zero_()
        self.regrets.zero_()
        if capture:
            self.graph = capture_on_side_stream(self._enqueue)
        torch.cuda.synchronize()

    def _enqueue(self, train: bool = True):
        """The six launches of one group update, on the current stream."""
        ops.bandit_rows_group(self.g_act)
        ops.mlp_group_fwd(self.g_fwd)
        ops.bandit_act_group(self.g_act)
        ops.bandit_replay_group(self.g_replay)
        if train:
            ops.mlp_group_train(self.g_train)

    def _step(self):
        if state.shard_samples:
            raise BnnHipError("GreedyBanditGroup: sample sharding is not supported")
        for opt in self.optimisers:
            opt.sync_lr()                        # what StepLR changed, into the device words (a fill, no host read)
        if self.graph is not None:
            self.graph.replay()
        else:
            self._enqueue()
        for s in self.schedulers:
            s.step()
        self.t += 1

    def update(self, mushroom: Optional[int] = None):
        """One bandit step of every agent (base_bandit.py:75-88 + main.py:103's scheduler.step()) on context `mushroom`,
        the same for all agents, or, when None, on a context each agent draws from its own stream.  Does not synchronise."""
        if self.t >= self.max_steps:
            raise BnnHipError(f"GreedyBanditGroup: max_steps={self.max_steps} reached")
        if mushroom is not None:
            i = int(mushroom)
            if not 0 <= i < self.N:
                raise BnnHipError(f"GreedyBanditGroup: context index {i} outside [0, {self.N})")
            self.indices[self.t].fill_(i)
        self._step()

    def run(self, indices: Sequence[int]):
        """update(i) for every i of `indices`, the sequence uploaded once."""
        idx = np.asarray(indices, dtype=np.int64).reshape(-1)
        if self.t + idx.size > self.max_steps:
            raise BnnHipError(f"GreedyBanditGroup: {idx.size} steps from step {self.t} pass max_steps={self.max_steps}")
        if idx.size and (idx.min() < 0 or idx.max() >= self.N):
            raise BnnHipError(f"GreedyBanditGroup: context indices must lie in [0, {self.N})")
        self.indices[self.t:self.t + idx.size].copy_(torch.from_numpy(idx))
        for _ in range(idx.size):
            self._step()

    def __len__(self):
        return self.G

    def __getitem__(self, g: int) -> "GreedyAgentView":
        if not -self.G <= g < self.G:
            raise IndexError(g)
        return GreedyAgentView(self, g % self.G)


class GreedyAgentView:
    """Agent g of a GreedyBanditGroup with BNNBandit's read surface.  Every read synchronises with the device once."""

    def __init__(self, group: GreedyBanditGroup, g: int):
        self.group, self.g = group, g
        self.label = f"{group.label}[{g}]"
        self.epsilon, self.seed = group.epsilons[g], group.seeds[g]
        self.net, self.optimiser, self.scheduler = group.nets[g], group.optimisers[g], group.schedulers[g]

    @property
    def t(self) -> int:
        return self.group.t

    @property
    def loss_info(self):
        """The loss of the last minibatch of the last update (mse_loss, sum): a float, or None before the first update."""
        return float(self.group.loss[self.g].item()) if self.group.t else None

    @property
    def cumulative_regrets(self) -> list:
        return self.group.regrets[self.g, :self.group.t + 1].tolist()

    @property
    def counts(self) -> np.ndarray:
        return self.group._counts[self.g].cpu().numpy()

    @property
    def tp(self) -> int:
        return int(self.group._counts[self.g, 1, 0].item())

    @property
    def fn(self) -> int:
        return int(self.group._counts[self.g, 1, 1].item())

    @property
    def fp(self) -> int:
        return int(self.group._counts[self.g, 0, 0].item())

    @property
    def tn(self) -> int:
        return int(self.group._counts[self.g, 0, 1].item())

    def history(self):
        """(actions [t] int64, rewards [t] fp32) of the steps taken, as numpy arrays."""
        t = self.group.t
        return self.group.actions[self.g, :t].cpu().numpy(), self.group.rewards[self.g, :t].cpu().numpy()


# ---------------------------------------------------------------------------------------------------- F7 BNN agents
def _per_agent(value, G: int, name: str) -> list:
    """`value` as a list of G: one value for all agents, or one per agent."""
    if isinstance(value, (str, bytes)) or not hasattr(value, "__len__"):
        return [value] * G
    if len(value) != G:
        raise BnnHipError(f"BNNBanditGroup: {len(value)} {name} for {G} seeds (one value, or one per agent)")
    return list(value)


class BNNBanditGroup:
    """G independent BNN_Bandit agents (bandits.py:17-54: a Bayes-by-Backprop network in-(hidden)-(hidden)-1 trained with
    Adam on sample_elbo, Thompson-sampling decisions) advanced together on the device.  One update of the whole group is
    six launches whatever G (include/bnn_hip.h F7), one workgroup per agent in each:

        bnn_bandit_rows_group -> bnn_bbb_group_fwd -> bnn_bandit_act_group -> bnn_bandit_replay_group (2)
        -> bnn_bbb_group_train (all nb minibatch steps of every agent)

    captured as one hipGraph (`capture=True`), kept as a recorded launch list (`"calls"`) or launched eagerly (`False`); the
    host never reads anything back.  The kernels are exact fp32 whatever bnn_hip.set_math says.

    G = len(seeds).  Agent g builds networks.BayesianNetwork exactly as BNN_Bandit.init_net does, in order under torch's RNG
    (a group of one after torch.manual_seed(k) starts where a BNNBandit built after the same call starts), with a capturable
    FusedAdam and StepLR(step_size=5000, gamma=0.5).  Its parameters and Adam's moments are views into the group's storage:
    `group[g].net` is a real network whose tensors the kernels update.  Per agent: the bandit's Philox stream (seeds[g]), the
    key of the network's epsilon stream (eps_seeds[g]; by default the global seed + g) with its own MC-sample counter starting
    at 0 (a sampled decision takes n_samples indices, then every minibatch n_samples: BNNBandit's sequence), epsilon, the
    decision rule (`policy`: "thompson" or "mean", as BNNBandit's) and the learning rate (bandit_params['lr']: one value or
    G).  n_samples, the prior and the shapes are the launch's: one for the group.
    update(mushroom) and run(indices) give every agent the same context, as main.py does; update() without an index lets each
    agent draw its context from its own stream.  `group[g]` is agent g's view (the BNNBandit read surface); every read
    synchronises."""

    def __init__(self, label, bandit_params, x, y, *, seeds, eps_seeds=None, epsilons=None, policy="thompson",
                 rewards: RewardTable = MUSHROOM, max_steps: int = 50000, local_reparam: bool = False, capture=True):
        p = bandit_params
        if state.shard_samples:
            raise BnnHipError("BNNBanditGroup: sample sharding is not supported (one device runs the whole loop)")
        if local_reparam or p.get("local_reparam", False):
            raise BnnHipError("BNNBanditGroup: local reparameterisation is not supported (its activation noise needs a "
                              "kernel of its own); BNNBandit(local_reparam=True, policy='mean') runs such a network")
        if p["mode"] != "regression":
            raise BnnHipError("BNNBanditGroup: the bandit's network regresses the reward (mode='regression')")
        if not (capture is True or capture is False or capture == "calls"):
            raise BnnHipError(f"BNNBanditGroup: capture must be True, 'calls' or False, got {capture!r}")
        self.label = label
        self.buffer_size, self.batch_size = int(p["buffer_size"]), int(p["batch_size"])
        self.num_batches, self.hidden, self.n_samples = int(p["num_batches"]), int(p["hidden_units"]), int(p["n_samples"])
        self.max_steps = int(max_steps)
        if self.batch_size < 1 or self.buffer_size % self.batch_size:
            raise BnnHipError("BNNBanditGroup: buffer_size must be a multiple of batch_size (the reference's last minibatch "
                              "is short)")
        if not hasattr(seeds, "__len__") or len(seeds) < 1:
            raise BnnHipError("BNNBanditGroup: seeds must be a non-empty list (one agent per seed)")
        self.G = len(seeds)
        self.seeds = [int(v) for v in seeds]
        if eps_seeds is not None and not hasattr(eps_seeds, "__len__"):
            raise BnnHipError("BNNBanditGroup: eps_seeds must be a list, one epsilon key per agent")
        self.eps_seeds = ([state.seed + g for g in range(self.G)] if eps_seeds is None
                          else [int(v) for v in _per_agent(eps_seeds, self.G, "eps_seeds")])
        self.epsilons = [float(e) for e in _per_agent(p["epsilon"] if epsilons is None else epsilons, self.G, "epsilons")]
        if any(not 0.0 <= e <= 1.0 for e in self.epsilons):                      # NaN fails the comparison
            raise BnnHipError(f"BNNBanditGroup: epsilons must lie in [0, 1], got {self.epsilons!r}")
        self.policies = _per_agent(policy, self.G, "policies")
        if any(q not in ("mean", "thompson") for q in self.policies):
            raise BnnHipError(f"BNNBanditGroup: policy must be 'mean' or 'thompson', got {policy!r}")
        self.lrs = [float(v) for v in _per_agent(p["lr"], self.G, "learning rates")]
        tab = np.asarray(rewards.rewards, dtype=np.float32)
        if tab.ndim != 3 or tab.shape[2] != 3 or tab.shape[1] < 2 or len(rewards.oracle) != tab.shape[0]:
            raise BnnHipError("BNNBanditGroup: rewards must be [K][A][(hi, lo, thr)] with A >= 2 and K oracle values")
        self.K, self.A = tab.shape[0], tab.shape[1]
        xh, yh = np.asarray(x, dtype=np.float32), np.asarray(y).astype(np.int64)
        if xh.ndim != 2 or yh.shape != (xh.shape[0],) or yh.min() < 0 or yh.max() >= self.K:
            raise BnnHipError("BNNBanditGroup: x must be [N, d] and y [N] labels in [0, K)")
        self.N, self.d = xh.shape
        W, H, S = self.d + self.A, self.hidden, self.n_samples
        nbm = self.buffer_size // self.batch_size
        if (W > L.MLP_GROUP_MAX_IN or not 1 <= H <= L.MLP_GROUP_MAX_HIDDEN or self.batch_size > L.MLP_GROUP_MAX_BATCH
                or nbm > L.MLP_GROUP_MAX_BATCHES or self.A > min(L.BANDIT_MAX_ACTIONS, L.MLP_GROUP_MAX_BATCH)
                or not 0 < self.buffer_size <= L.BANDIT_MAX_BUFFER or self.G > L.MLP_GROUP_MAX_AGENTS or self.max_steps < 1
                or not 1 <= S <= L.BBB_GROUP_MAX_SAMPLES):
            raise BnnHipError(f"BNNBanditGroup: beyond the kernels' limits (input {W} <= {L.MLP_GROUP_MAX_IN}, hidden <= "
                              f"{L.MLP_GROUP_MAX_HIDDEN}, batch <= {L.MLP_GROUP_MAX_BATCH}, buffer / batch <= "
                              f"{L.MLP_GROUP_MAX_BATCHES}, buffer <= {L.BANDIT_MAX_BUFFER}, agents <= {L.MLP_GROUP_MAX_AGENTS}, "
                              f"1 <= n_samples <= {L.BBB_GROUP_MAX_SAMPLES})")

        import networks
        dev = torch.device("cuda", torch.cuda.current_device())
        self.x = torch.from_numpy(xh).to(dev).contiguous()
        self.y = torch.from_numpy(yh).to(dev)
        self.table = torch.from_numpy(tab).to(dev)
        self.oracle = torch.tensor(rewards.oracle, dtype=torch.float32, device=dev)

        # bandits.py:23-37, agent by agent; the parameters and Adam's moments become views of one [G, P] tensor each
        model_params = {'input_shape': W, 'classes': 1, 'batch_size': self.batch_size, 'hidden_units': H, 'mode': p['mode'],
                        'mixture_prior': p['mixture_prior'], 'mu_init': p['mu_init'], 'rho_init': p['rho_init'],
                        'prior_init': p['prior_init'], 'local_reparam': False}
        G, T, B = self.G, self.max_steps, self.buffer_size
        i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
        self.nets = [networks.BayesianNetwork(model_params) for _ in range(G)]
        P = sum(q.numel() for q in self.nets[0].parameters())
        self.param_store, self.exp_avg, self.exp_avg_sq = torch.zeros((G, P), **f32), torch.zeros((G, P), **f32), \
            torch.zeros((G, P), **f32)
        self.prior = self.nets[0].l1._prior_spec
        self.optimisers, self.schedulers = [], []
        for g, net in enumerate(self.nets):
            off = 0
            for q in net.parameters():
                n = q.numel()
                view = self.param_store[g, off:off + n].view(q.shape)
                view.copy_(q.data)
                q.data = view
                off += n
            opt = FusedAdam(net.parameters(), lr=self.lrs[g], capturable=True)
            off = 0
            for q in net.parameters():                                            # Adam's state, as its first step makes it
                n = q.numel()
                st = opt.state[q]
                st["step"] = 0
                st["exp_avg"] = self.exp_avg[g, off:off + n].view(q.shape)
                st["exp_avg_sq"] = self.exp_avg_sq[g, off:off + n].view(q.shape)
                off += n
            self.optimisers.append(opt)
            self.schedulers.append(torch.optim.lr_scheduler.StepLR(opt, step_size=5000, gamma=0.5))

        # device state, [G, ...] with one contiguous row per agent
        self.step_word = torch.zeros((G, 1), **i32)
        self.cur_index = torch.zeros((G, 1), **i32)
        self.indices = torch.full((T,), -1, dtype=torch.int64, device=dev)       # shared: -1 = each agent draws its own
        self.actions = torch.zeros((G, T), dtype=torch.int64, device=dev)
        self.rewards = torch.zeros((G, T), **f32)
        self.regrets = torch.zeros((G, T + 1), dtype=torch.float64, device=dev)
        self._counts = torch.zeros((G, self.K, self.A), dtype=torch.int64, device=dev)
        self.ring_index, self.ring_action, self.ring_reward = torch.zeros((G, B), **i32), torch.zeros((G, B), **i32), \
            torch.zeros((G, B), **f32)
        self.perm = torch.zeros((G, B), **i32)
        self.nb_slab = nbm
        self.slab = torch.zeros((G, nbm, self.batch_size, W), **f32)
        self.targets = torch.zeros((G, nbm, self.batch_size), **f32)
        self.n_batches_word = torch.zeros((G, 1), **i32)
        self.loss = torch.zeros((G, 4), **f32)                                   # (loss, log_p, log_q, nll) per agent
        self.rows = torch.zeros((G, self.A, W), **f32)
        self.outputs = torch.zeros((G, S, self.A), **f32)
        self.sample_counter = torch.zeros((G, 1), **i32)
        self.workspace = torch.zeros((G, ops.bbb_group_workspace_bytes(W, H) // 4), **f32)
        self.t = 0

        act, rep, bbb = [], [], []
        for g in range(G):
            thompson = self.policies[g] == "thompson"
            act.append(ops.bandit_act_args(
                x=self.x, labels=self.y, rewards=self.table, oracle=self.oracle, outputs=self.outputs[g], n_samples=S,
                output_sample_stride=self.A if thompson else 0, step=self.step_word[g], cur_index=self.cur_index[g],
                rows=self.rows[g], actions=self.actions[g], reward_out=self.rewards[g], regrets=self.regrets[g],
                counts=self._counts[g], ring_index=self.ring_index[g], ring_action=self.ring_action[g],
                ring_reward=self.ring_reward[g], epsilon=self.epsilons[g], seed=self.seeds[g], indices=self.indices,
                sample_counter=self.sample_counter[g] if thompson else None, sample_counter_inc=S if thompson else 0))
            rep.append(ops.bandit_replay_args(
                x=self.x, step=self.step_word[g], ring_index=self.ring_index[g], ring_action=self.ring_action[g],
                ring_reward=self.ring_reward[g], workspace=self.perm[g], slab=self.slab[g], targets=self.targets[g],
                batch_size=self.batch_size, n_actions=self.A, seed=self.seeds[g], n_batches=self.n_batches_word[g]))
            opt = self.optimisers[g]
            qs = list(self.nets[g].parameters())
            step_dev, lr_dev, _, _ = opt._group_dev(0, opt.param_groups[0], dev)
            bbb.append(ops.bbb_group_agent(
                params=[q.detach() for q in qs], exp_avg=[opt.state[q]["exp_avg"] for q in qs],
                exp_avg_sq=[opt.state[q]["exp_avg_sq"] for q in qs], step=step_dev, lr=lr_dev, slab=self.slab[g],
                targets=self.targets[g], n_batches=self.n_batches_word[g], loss_info=self.loss[g], rows=self.rows[g],
                outputs=self.outputs[g], sample_counter=self.sample_counter[g], workspace=self.workspace[g],
                eps_seed=self.eps_seeds[g], eps_mode=L.EPS_PHILOX if thompson else L.EPS_ZERO))
        grp = self.optimisers[0].param_groups[0]
        self.g_act = ops.bandit_group_args(act, dev)
        self.g_replay = ops.bandit_group_args(rep, dev)
        shape = dict(in_features=W, hidden=H, n_samples=S, device=dev, prior=self.prior, betas=grp["betas"], eps=grp["eps"],
                     weight_decay=grp["weight_decay"])
        self.g_fwd = ops.bbb_group_args(bbb, n_rows=self.A, **shape)
        self.g_train = ops.bbb_group_args(bbb, batch=self.batch_size, max_batches=nbm,
                                          kl_weights=[beta(j, self.num_batches) for j in range(nbm)], **shape)

        # warm-up: every launch once, eagerly (this validates every block), recorded for capture="calls"; the training
        # launch runs with nb = 0 and touches nothing.  Then the words the warm-up moved are reset, and the update is captured.
        self.capture = capture
        self.graph = self.calls = None
        with L.recording() as calls:
            self._enqueue(train=False)
        recorded = list(calls)
        self.n_batches_word.zero_()
        with L.recording() as calls:
            ops.bbb_group_train(self.g_train)
        recorded += list(calls)
        if capture == "calls":
            self.calls = recorded
        torch.cuda.synchronize()
        self.step_word.zero_()
        self._counts.zero_()
        self.regrets.zero_()
        self.sample_counter.zero_()
        if capture is True:
            self.graph = capture_on_side_stream(self._enqueue)
        torch.cuda.synchronize()

    def _enqueue(self, train: bool = True):
        """The six launches of one group update, on the current stream."""
        ops.bandit_rows_group(self.g_act)
        ops.bbb_group_fwd(self.g_fwd)
        ops.bandit_act_group(self.g_act)
        ops.bandit_replay_group(self.g_replay)
        if train:
            ops.bbb_group_train(self.g_train)

    def _step(self):
        if state.shard_samples:
            raise BnnHipError("BNNBanditGroup: sample sharding is not supported")
        for opt in self.optimisers:
            opt.sync_lr()                        # what StepLR changed, into the device words (a fill, no host read)
        if self.graph is not None:
            self.graph.replay()
        elif self.calls is not None:
            BNNBandit._run_calls(self.calls)
        else:
            self._enqueue()
        for s in self.schedulers:
            s.step()
        self.t += 1

    def update(self, mushroom: Optional[int] = None):
        """One bandit step of every agent (base_bandit.py:75-88 + main.py:103's scheduler.step()) on context `mushroom`,
        the same for all agents, or, when None, on a context each agent draws from its own stream.  Does not synchronise."""
        if self.t >= self.max_steps:
            raise BnnHipError(f"BNNBanditGroup: max_steps={self.max_steps} reached")
        if mushroom is not None:
            i = int(mushroom)
            if not 0 <= i < self.N:
                raise BnnHipError(f"BNNBanditGroup: context index {i} outside [0, {self.N})")
            self.indices[self.t].fill_(i)
        self._step()

    def run(self, indices: Sequence[int]):
        """update(i) for every i of `indices`, the sequence uploaded once."""
        idx = np.asarray(indices, dtype=np.int64).reshape(-1)
        if self.t + idx.size > self.max_steps:
            raise BnnHipError(f"BNNBanditGroup: {idx.size} steps from step {self.t} pass max_steps={self.max_steps}")
        if idx.size and (idx.min() < 0 or idx.max() >= self.N):
            raise BnnHipError(f"BNNBanditGroup: context indices must lie in [0, {self.N})")
        if idx.size:
            self._staged = torch.from_numpy(idx).pin_memory()    # kept until the next run(): the copy does not wait for the host
            self.indices[self.t:self.t + idx.size].copy_(self._staged, non_blocking=True)
        for _ in range(idx.size):
            self._step()

    def __len__(self):
        return self.G

    def __getitem__(self, g: int) -> "BNNAgentView":
        if not -self.G <= g < self.G:
            raise IndexError(g)
        return BNNAgentView(self, g % self.G)


class BNNAgentView(GreedyAgentView):
    """Agent g of a BNNBanditGroup with BNNBandit's read surface.  Every read synchronises with the device once."""

    def __init__(self, group: BNNBanditGroup, g: int):
        super().__init__(group, g)
        self.eps_seed, self.policy, self.n_samples = group.eps_seeds[g], group.policies[g], group.n_samples

    @property
    def loss_info(self):
        """(loss, mean log_p, mean log_q, mean nll) of the last minibatch of the last update (sample_elbo's tuple, as
        floats), or None before the first update."""
        return tuple(self.group.loss[self.g].tolist()) if self.group.t else None

    @property
    def sample_counter(self) -> int:
        """The next unused MC-sample index of the agent's epsilon stream."""
        return int(self.group.sample_counter[self.g].item()) & 0xFFFFFFFF


class GreedyBandit(GreedyAgentView):
    """Greedy_Bandit (bandits.py:59-85) on the device: a GreedyBanditGroup of one, with the reference's constructor arguments
    (epsilon from bandit_params) -- a drop-in where main.py:91-93 builds one.  update() / run() as the group's."""

    def __init__(self, label, bandit_params, x, y, *, seed: Optional[int] = None, rewards: RewardTable = MUSHROOM,
                 max_steps: int = 50000, capture: bool = True):
        group = GreedyBanditGroup(label, bandit_params, x, y, epsilons=[bandit_params["epsilon"]],
                                  seeds=None if seed is None else [seed], rewards=rewards, max_steps=max_steps, capture=capture)
        super().__init__(group, 0)
        self.label = label
        self.n_samples = int(bandit_params.get("n_samples", 1))
        self.buffer_size, self.batch_size = group.buffer_size, group.batch_size
        self.num_batches, self.lr = group.num_batches, group.lr

    def update(self, mushroom: Optional[int] = None):
        self.group.update(mushroom)

    def run(self, indices: Sequence[int]):
        self.group.run(indices)
