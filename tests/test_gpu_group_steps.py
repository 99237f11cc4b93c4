"""The grouped bandit kernels (include/bnn_hip.h F6 bnn_mlp_group_*, F7 bnn_bbb_group_*) against the float64 restatement of one
launch (tests/group_ref.py) across their ABI: a. one or two minibatch steps from a loaded Adam state (step 7, non-zero moments)
with non-default betas / eps / weight decay, Gaussian and mixture priors, S = 1, 2, 8, from 1-1-1 at batch 1 to 128-128-1 at
batch 64; b. the decision forwards at 1, 5 and 64 rows; c. a chain of max_batches = 128 minibatches against 128 launches of one,
bit for bit; d. the n_batches word (0, negative, above max_batches) and per-agent lr / step words in one launch; e. guard words
around every tensor a launch may write (in a. and b.).

Bounds (tests/group_ref.py, tests/test_group_ref_cpu.py): per tensor class, relative to each tensor's max |.|,
min(max(4 d_ref, n 2^-23), 2e-4), d_ref the deviation of a numpy fp32 restatement (numpy's summation order) from the float64
reference, computed here at run time on the device's own epsilon; n the class's operation count (group_ref.FLOOR_OPS).

Measured on an MI355X (d_ref on the device's epsilon / bound used / the kernel's deviation; * = the bound is the operation-count
floor n 2^-23, with n = 21, 14, 15, 6 for F6's parameters, exp_avg, exp_avg_sq, outputs and 30, 23, 24, 10 for F7's; no case
reached the 2e-4 cap):
  a. steps                        parameters                      exp_avg                         exp_avg_sq
  f6 1-1-1 b1                     1.58e-6  6.33e-6  2.48e-6       8.44e-8  1.67e-6* 8.44e-8       3.98e-8  1.79e-6* 3.98e-8
  f6 5-7-7-1 b3                   3.81e-8  2.50e-6* 3.81e-8       2.17e-7  1.67e-6* 2.17e-7       7.12e-8  1.79e-6* 6.60e-8
  f6 37-19-19-1 b8                4.55e-8  2.50e-6* 4.53e-8       1.04e-7  1.67e-6* 1.13e-7       1.94e-7  1.79e-6* 1.77e-7
  f6 37-19-19-1 b8, default Adam  4.45e-8  2.50e-6* 4.45e-8       5.32e-8  1.67e-6* 8.23e-8       1.21e-7  1.79e-6* 1.63e-7
  f6 128-128-128-1 b64            4.43e-8  2.50e-6* 4.43e-8       1.71e-6  6.86e-6  2.82e-6       4.08e-7  1.79e-6* 4.08e-7
  f7 1-1-1 b1 S1 gauss            4.79e-8  3.58e-6* 4.79e-8       2.54e-6  1.02e-5  3.77e-6       6.93e-8  2.86e-6* 6.93e-8
  f7 5-7-7-1 b3 nb2 S8 mixture    8.79e-8  3.58e-6* 8.79e-8       9.23e-7  3.69e-6  2.01e-6       1.26e-6  5.05e-6  2.27e-6
  f7 37-19-19-1 b8 nb2 S2 gauss   9.46e-8  3.58e-6* 9.46e-8       1.06e-7  2.74e-6* 1.22e-7       1.43e-7  2.86e-6* 2.07e-7
  f7 37-19 b8 S2 mix, default     4.88e-8  3.58e-6* 4.88e-8       1.46e-6  5.85e-6  2.24e-6       4.00e-6  1.60e-5  5.97e-6
  f7 128-128-128-1 b64 S2 mix     4.79e-8  3.58e-6* 4.79e-8       8.84e-7  3.58e-6  2.49e-6       9.69e-7  3.88e-6  3.53e-6
  (The parameters move by about lr = 1e-3 in one step, so their deviation is mostly the final p - step_size (m / denom) rounding,
  the same in the kernel and in the restatement; the moments carry the gradient's arithmetic.  F7's moments are widest where
  sum_s t_s eps_s and beta / sigma nearly cancel in g_rho; the closest any tensor comes to its bound is F7's exp_avg_sq at
  128-128-128-1, 0.91 of it.)  The loss words are held to group_ref.loss_tolerance: F6's loss to 3e-7 .. 8e-6 of itself, F7's
  (loss, log_p, log_q, nll) to at most 1.2e-5 of the loss; the kernels' agreed with float64 to the seven digits printed.
  b. forwards, outputs: F6 d_ref 4.4e-8 .. 2.1e-7, bound 7.15e-7* (8.57e-7 at 37-19 with 64 rows), the kernel 5.2e-8 .. 3.97e-7
  (128-128, 5 rows); F7 d_ref 5.7e-9 .. 4.5e-7, bound 1.19e-6* (1.3e-6 .. 1.8e-6 at 128-128 with 1 row, or 64 rows and 8 draws),
  the kernel 1.7e-8 .. 6.68e-7 (128-128, 5 rows, EPS_ZERO).
  c., d. torch.equal throughout; no guard word changed anywhere.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import group_ref as R
from bnn_hip import _lib as L
from bnn_hip import ops
from oracle import bnn_oracle as O

PATTERN = 0x5A5AA5A5                   # the guard words' bits (an fp32 of about 1.5e16: a stray read of it would show, too)
GUARD = 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


class _Guarded:
    """Tensors carved from buffers with GUARD words of PATTERN on either side."""

    def __init__(self, dev):
        self.dev, self.bufs = dev, []

    def make(self, name, value, dtype=torch.float32):
        value = np.asarray(value)
        n = value.size
        buf = torch.full((n + 2 * GUARD,), PATTERN, dtype=torch.int32, device=self.dev)
        self.bufs.append((name, buf, n))
        t = buf[GUARD:GUARD + n].view(dtype).view(value.shape)
        t.copy_(torch.from_numpy(value.astype(np.float32 if dtype == torch.float32 else np.int32)))
        return t

    def check(self):
        for name, buf, n in self.bufs:
            assert bool((buf[:GUARD] == PATTERN).all()), f"{name}: the words below it were written"
            assert bool((buf[GUARD + n:] == PATTERN).all()), f"{name}: the words above it were written"


class _Agent:
    """One agent's device tensors from group_ref's float32 inputs, every writable one guarded."""

    def __init__(self, case, inp, dev, *, nb=None, lr=None, step0=None, fill_ws=0.0):
        g = self.guard = _Guarded(dev)
        self.case = case
        f7 = case.kind == "f7"
        self.params = [g.make(f"param[{i}]", p) for i, p in enumerate(inp["params"])]
        zeros = [np.zeros_like(p) for p in inp["params"]]
        self.m = [g.make(f"exp_avg[{i}]", p) for i, p in enumerate(inp.get("exp_avg", zeros))]
        self.v = [g.make(f"exp_avg_sq[{i}]", p) for i, p in enumerate(inp.get("exp_avg_sq", zeros))]
        self.step = g.make("step", [case.step0 if step0 is None else step0], torch.int32)
        self.lr = torch.tensor([case.lr if lr is None else lr], dtype=torch.float32, device=dev)
        self.nbw = torch.tensor([case.nb if nb is None else nb], dtype=torch.int32, device=dev)
        self.loss = g.make("loss", [123.0] * (4 if f7 else 1))
        self.slab = torch.from_numpy(inp["slab"]).to(dev) if "slab" in inp else None
        self.targets = torch.from_numpy(inp["targets"]).to(dev) if "targets" in inp else None
        self.rows = torch.from_numpy(inp["rows"]).to(dev) if "rows" in inp else None
        self.out = None
        if self.rows is not None:
            ns = 1 if (not f7 or case.zero_eps) else case.S
            self.out = g.make("outputs", np.zeros((ns, case.B) if f7 else (case.B,)))
        if f7:
            self.counter = g.make("sample_counter", [case.counter], torch.int32)
            self.ws = g.make("workspace", np.full(ops.bbb_group_workspace_bytes(case.I, case.H) // 4, fill_ws))
            assert self.ws.data_ptr() % 16 == 0

    def block(self, slab=None, targets=None):
        c = self.case
        slab, targets = self.slab if slab is None else slab, self.targets if targets is None else targets
        common = dict(params=self.params, exp_avg=self.m, exp_avg_sq=self.v, step=self.step, lr=self.lr, slab=slab, targets=targets,
                      n_batches=self.nbw, rows=self.rows, outputs=self.out)
        if c.kind == "f6":
            return ops.mlp_group_agent(loss=self.loss, **common)
        return ops.bbb_group_agent(loss_info=self.loss, sample_counter=self.counter, workspace=self.ws, eps_seed=c.eps_seed,
                                   eps_mode=L.EPS_ZERO if c.zero_eps else L.EPS_PHILOX, **common)

    def state(self):
        """Every tensor and word a launch may write, on the host."""
        out = [t.cpu().clone() for t in self.params + self.m + self.v] + [self.step.cpu().clone(), self.loss.cpu().clone()]
        if self.case.kind == "f7":
            out.append(self.counter.cpu().clone())
        return out


def _train_args(case, blocks, dev, *, max_batches, kl=None):
    shape = dict(in_features=case.I, hidden=case.H, device=dev, batch=case.B, max_batches=max_batches, betas=case.betas,
                 eps=case.eps, weight_decay=case.wd)
    if case.kind == "f6":
        return ops.mlp_group_args(blocks, **shape)
    return ops.bbb_group_args(blocks, n_samples=case.S, prior=ops.PriorSpec.from_init(list(case.prior_init), case.mixture),
                              kl_weights=list(case.kl if kl is None else kl)[:max_batches], **shape)


def _train(case, args):
    (ops.mlp_group_train if case.kind == "f6" else ops.bbb_group_train)(args)


def _device_eps(case, dev):
    """group_ref's eps(layer, kind, first, S, rows, cols) from the device's own materialised stream, widened to float64."""
    def f(layer, kind, first, S, rows, cols):
        return ops.philox_normal(case.eps_seed, O.tensor_id(layer, kind), first & 0xFFFFFFFF, S, rows, cols, dev).cpu().numpy() \
            .astype(np.float64)
    return f


def _same_state(a, b, what):
    for i, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), (what, i)


# ---------------------------------------------------------------------------------------------------- a. (and e.) one step
@pytest.mark.parametrize("case", R.STEP_CASES, ids=lambda c: c.id)
def test_steps_match_float64(dev, case):
    inp = R.inputs(case)
    eps_fn = _device_eps(case, dev) if case.kind == "f7" else None
    ref = R.step64(case, inp, eps_fn)
    dref = R.d_ref(case, inp, ref, eps_fn)
    bnds = R.bounds(case, dref)
    ag = _Agent(case, inp, dev)
    _train(case, _train_args(case, [ag.block()], dev, max_batches=case.nb))
    torch.cuda.synchronize()
    print(f"  {case.id}")
    worst = dict.fromkeys(("params", "exp_avg", "exp_avg_sq"), 0.0)
    fails = []
    for c, got in (("params", ag.params), ("exp_avg", ag.m), ("exp_avg_sq", ag.v)):
        for i, t in enumerate(got):
            d = R.rel_dev(t.cpu().numpy(), ref[c][i])
            worst[c] = max(worst[c], d)
            if d > bnds[c]:
                fails.append((c, i, d, bnds[c]))
        print(f"    {c}: deviation {worst[c]:.3e} of a tensor's scale (d_ref {dref[c]:.3e}, bound {bnds[c]:.3e})")
    tol = R.loss_tolerance(case, inp, ref, bnds)
    if case.kind == "f6":
        loss = float(ag.loss)
        print(f"    loss {loss:.7g} vs {ref['loss']:.7g} (bound {tol:.3e})")
        assert abs(loss - ref["loss"]) <= tol
    else:
        info = ag.loss.cpu().numpy().astype(np.float64)
        print("    loss_info (loss, log_p, log_q, nll) " + "; ".join(f"{a:.7g} vs {b:.7g} (bound {t:.3e})"
                                                                      for a, b, t in zip(info, ref["loss_info"], tol)))
        assert (np.abs(info - ref["loss_info"]) <= tol).all()
        assert int(ag.counter) == ref["counter"]
    assert not fails, fails
    assert int(ag.step) == ref["step"]
    ag.guard.check()


# ---------------------------------------------------------------------------------------------------- b. (and e.) forwards
@pytest.mark.parametrize("case", R.FWD_CASES, ids=lambda c: c.id)
def test_decision_forwards_match_float64(dev, case):
    inp = R.inputs(case, train=False)
    f7 = case.kind == "f7"
    eps_fn = _device_eps(case, dev) if f7 else None
    ref = R.forward64(case, inp, eps_fn)
    dref = R.d_ref(case, inp, ref, eps_fn, train=False)
    bnd = R.bounds(case, dref)["outputs"]
    ag = _Agent(case, inp, dev)
    before = ag.state()
    shape = dict(in_features=case.I, hidden=case.H, device=dev, n_rows=case.B)
    if f7:
        ops.bbb_group_fwd(ops.bbb_group_args([ag.block()], n_samples=case.S, **shape))
    else:
        ops.mlp_group_fwd(ops.mlp_group_args([ag.block()], **shape))
    torch.cuda.synchronize()
    d = R.rel_dev(ag.out.cpu().numpy(), ref["z"] if f7 else ref["z"][0])
    print(f"  {case.id}: deviation {d:.3e} of the scale (d_ref {dref['outputs']:.3e}, bound {bnd:.3e})")
    assert d <= bnd
    _same_state(ag.state(), before, "a forward writes its outputs and workspace only")       # the counter is read, not advanced
    if f7 and not case.zero_eps and case.S > 1:
        assert float(np.abs(ref["z"][0] - ref["z"][1]).max()) > 0
    ag.guard.check()


# ---------------------------------------------------------------------------------------------------- c. a chain is its steps
def _chain_case(kind, I, H, B, nb):
    kl = tuple(float(np.float32(0.9 * (nb - j) / (nb * (nb + 1) / 2))) for j in range(nb))      # nb distinct KL weights
    return R.Case(kind, I, H, B, nb=nb, S=2, kl=kl, seed=2, **R.MIX)


@pytest.mark.parametrize("kind", ["f6", "f7"])
@pytest.mark.parametrize("I,H,B,nb", [(5, 7, 3, L.MLP_GROUP_MAX_BATCHES), (119, 100, 64, 8)])
def test_a_chain_is_its_steps_bit_for_bit(dev, kind, I, H, B, nb):
    """One launch of nb minibatches against nb launches of one over the same slab rows, each with its own beta[0] = beta_j and
    the step word and sample counter carried over on the device: pins beta[j], t = step + j + 1 and c + j S + s at every j."""
    case = _chain_case(kind, I, H, B, nb)
    assert len(set(case.kl)) == nb
    inp = R.inputs(case)
    whole, single = _Agent(case, inp, dev), _Agent(case, inp, dev, nb=1)
    _train(case, _train_args(case, [whole.block()], dev, max_batches=nb))
    for j in range(nb):
        blk = single.block(slab=single.slab[j], targets=single.targets[j])
        _train(case, _train_args(case, [blk], dev, max_batches=1, kl=[case.kl[j]]))
    torch.cuda.synchronize()
    assert int(whole.step) == case.step0 + nb
    if kind == "f7":
        assert int(whole.counter) == case.counter + nb * case.S
    assert all(not torch.equal(p, torch.from_numpy(q)) for p, q in zip(whole.state(), inp["params"]))       # it trained
    _same_state(whole.state(), single.state(), f"{kind} {I}-{H} batch {B}: {nb} minibatches")
    whole.guard.check()
    single.guard.check()


# ---------------------------------------------------------------------------------------------------- d. the n_batches word
@pytest.mark.parametrize("kind", ["f6", "f7"])
def test_n_batches_word_and_per_agent_words(dev, kind):
    """Four agents of one launch with *n_batches = 0, -3, 2 and max_batches + 5 (max_batches = 3), their own lr and start step:
    0 and negative write nothing (every tensor and word, the loss words and the workspace too), 2 is a launch of 2, above
    max_batches is a launch of max_batches."""
    mb = 3
    base = R.Case(kind, 5, 7, 3, nb=mb, S=2, kl=(0.37, 0.11, 0.23), **R.MIX)
    words = [0, -3, 2, mb + 5]
    lrs, steps = [1e-3, 2e-3, 3e-3, 5e-4], [7, 0, 11, 100]
    cases = [R.with_seed(base, 3 + g) for g in range(4)]
    inps = [R.inputs(c) for c in cases]
    agents = [_Agent(c, i, dev, nb=w, lr=lr, step0=s, fill_ws=-7.0) for c, i, w, lr, s in zip(cases, inps, words, lrs, steps)]
    before = [a.state() for a in agents]
    _train(base, _train_args(base, [a.block() for a in agents], dev, max_batches=mb))
    torch.cuda.synchronize()
    for g in (0, 1):
        _same_state(agents[g].state(), before[g], f"agent {g} (*n_batches = {words[g]}) must be untouched")
        if kind == "f7":
            assert bool((agents[g].ws == -7.0).all()), g
    for g, n in ((2, 2), (3, mb)):
        alone = _Agent(cases[g], inps[g], dev, nb=n, lr=lrs[g], step0=steps[g])
        _train(base, _train_args(base, [alone.block()], dev, max_batches=mb))
        torch.cuda.synchronize()
        assert int(alone.step) == steps[g] + n
        _same_state(agents[g].state(), alone.state(), f"agent {g} (*n_batches = {words[g]}) against a launch of {n}")
    for a in agents:
        a.guard.check()
