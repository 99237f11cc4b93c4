"""The F14 sparse training step on an MI355X (bnn_sparse_elbo_terms, bnn_sparse_bwd, bnn_sparse_sigma_refresh;
posthoc.CompressedNetwork.graphed_train_step -> sparse_train.SparseTrainStep): the gradients and the ELBO scalars against the
fp64 restatement of tests/sparse_train_ref.py on the step's own inputs, level 0 against the dense GraphedTrainStep, Adam and
the sigma refresh bit for bit, the fixed pattern, reproducibility (two objects, replay against eager launches, a build that
leaves no trace), an EpochRunner, and a short fine-tuning run.

The tolerance of every comparison with fp64 is 4 x REF32 of the case, REF32 being the deviation of the restatement's own
fp32 form (numpy's summation orders) from its fp64 form on the same inputs: two independent fp32 orderings and a factor 2 for
the chain of three layers and two passes, as tests/test_gpu_bnn_bandit_group.py argues; 4 x REF32 may not exceed 2e-4 (the
project's F6 bound) -- a case where it does fails instead of loosening.

Case 2 (1-48-1 at 98 %) has no path from the input to the output left, whatever the parameter seed: the data term of every
gradient is exactly zero there (tests/test_sparse_train_cpu.py asserts it, DATA_DEAD), so that case checks the weight-gradient
dots against zeros plus the complexity term (regenerated epsilon, prior, log q); for the 1-48-1 net the data term is checked
by cases 0 and 1 alone.

Measured on an MI355X (worst tensor of each case, relative to the tensor's max |.|; step 1 / step 2):
  case 0             kernel 3.649e-07 / 3.002e-07   REF32 2.792e-07 / 2.186e-07
  case 1             kernel 3.564e-07 / 3.791e-07   REF32 1.066e-06 / 3.740e-07
  case 2             kernel 3.011e-07 / 3.709e-07   REF32 1.768e-07 / 2.129e-07
  case 3             kernel 2.682e-07 / 2.364e-07   REF32 4.653e-07 / 4.031e-07
  case 4             kernel 3.621e-07 / 3.318e-07   REF32 2.430e-07 / 2.713e-07
  case 5             kernel 3.813e-07 / 3.624e-07   REF32 7.263e-07 / 3.164e-07
  case 6             kernel 3.437e-07 / 2.508e-07   REF32 2.373e-07 / 2.273e-07
  case 7             kernel 3.120e-07 / 3.873e-07   REF32 2.399e-07 / 2.898e-07
  case 8             kernel 3.687e-07 / 3.712e-07   REF32 2.593e-07 / 2.666e-07
  case 9             kernel 4.969e-07 / 2.761e-07   REF32 9.632e-07 / 7.489e-07
  empty row lr=False kernel 3.779e-07 / 3.668e-07   REF32 2.701e-07 / 2.619e-07
  empty row lr=True  kernel 3.984e-07 / 3.944e-07   REF32 2.365e-07 / 5.470e-07
  empty layers       kernel 3.041e-07 / 3.865e-07   REF32 2.257e-07 / 1.395e-07
  level 0 against the dense step (f32 math): at most 1.7e-07 of a tensor's scale (Gaussian), 1.1e-07 (mixture)
  fine-tuning at 75 %: mean loss of the first 20 steps 7545.4, of the last 20 7049.6
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bnn_hip
import sparse_train_ref as R
from bnn_hip import _lib as L, ops, posthoc, synth
from bnn_hip.epoch import DeviceDataset, DeviceLoader, EpochRunner, beta_table
from bnn_hip.optim import FusedAdam
from bnn_hip.runtime import manual_seed, state
from bnn_hip.train import GraphedTrainStep
from test_sparse_cpu import chain_bound_layer, sparse_forward_ref, sparse_layer_ref

SEED = 2026
F6_BOUND = 2e-4
FWD_TOL = 1e-5                                  # of the output scale: the whole-network bound of tests/test_gpu_sparse.py
MIX = [0.5, 0, -6]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _math_back():
    bnn_hip.set_math("f32")
    yield
    bnn_hip.set_math("bf16")


def _net(dims, mode, lr, mixture, dev, param_seed=synth.SEED_PARAMS):
    import networks
    mp = dict(input_shape=dims[0], classes=dims[2], batch_size=128, hidden_units=dims[1], mode=mode, mu_init=[-0.2, 0.2],
              rho_init=[-5, -4], prior_init=MIX if mixture else [1.0], mixture_prior=bool(mixture), local_reparam=lr)
    net = networks.BayesianNetwork(mp)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(*dims, lr, seed=param_seed).items()})
    return net.to(dev).train()


def _batch(mode, rows, dims, dev, seed=5):
    x, y = synth.synth_batch(mode, rows, dims[0], dims[2], seed=seed)
    return torch.from_numpy(x.reshape(rows, -1)).to(dev), torch.from_numpy(y).to(dev)


def _step(cn, x, y, S, lr=1e-3, **kw):
    """A step object on a fresh optimiser, the epsilon stream rewound: global sample indices 0, 1, ..."""
    manual_seed(SEED, 0)
    opt = FusedAdam(cn.parameters(), lr=lr, capturable=True)
    return cn.graphed_train_step(opt, x, y, S, **kw), opt


def _np(t):
    return t.detach().cpu().numpy()


def _case_of(step, beta):
    """The restatement's case of the step's CURRENT state: its parameters, its sigma (the device's bits), its minibatch and
    the global index of its next sample."""
    cn = step.cn
    layers = []
    for c, keep in zip(cn._layers, step.keep):
        rp = _np(c.row_ptr)
        rows = np.repeat(np.arange(c.fout), np.diff(rp)).astype(np.int64)
        n = c.nnz
        layers.append(dict(row_ptr=rp, col=(_np(c.col)[:n].view(np.uint16)).astype(np.int64), rows=rows, mu_val=_np(c.mu_val)[:n],
                           rho_val=_np(c.rho_val)[:n], sigma_val=_np(c.sigma_val)[:n], b_mu=_np(c.b_mu), b_rho=_np(c.b_rho),
                           b_sigma=_np(c.b_sigma), b_keep=_np(keep), fin=c.fin, fout=c.fout, layer_id=c.layer_id))
    pr = step.prior
    first = (step.base + step._shared["mirror"]) & 0xFFFFFFFF
    return dict(layers=layers, x=_np(step.x), y=_np(step.y), mode=cn.mode, S=step.samples, first=first, seed=state.seed,
                beta=float(np.float32(beta)), prior=dict(mixture=pr.mixture, sigma_p=pr.sigma_p, pi=pr.pi, sigma1=pr.sigma1,
                                                         sigma2=pr.sigma2), nll_sigma=step.sigma)


def _grads(step):
    return [_np(g).copy() for g in step.grad_views]


def _out4(out):
    return np.array([float(o.reshape(-1)[0]) for o in out])


def _check_against_fp64(step, x, y, beta, label):
    """One step: its bucket and out4 against the fp64 closed forms on the state the step started from."""
    case = dict(_case_of(step, beta), x=_np(x), y=_np(y))                 # (the minibatch is staged by the step below)
    ref = R.closed_ref(case, np.float64)
    r32 = R.ref32_of(case, ref)
    tol = 4 * r32
    for i, l in enumerate(case["layers"]):                                # the comparison is not vacuous
        if len(l["col"]):
            assert np.any(ref[1][4 * i] != 0) and np.any(ref[1][4 * i + 1] != 0)
    out = _out4(step.step(x, y, beta))
    got = _grads(step)
    devs = [R.rel_dev(out, ref[0])] + [R.rel_dev(a, b) for a, b in zip(got, ref[1])]
    worst = int(np.argmax(devs))
    print(f"{label}: kernel {max(devs):.3e} ({(('out4',) + R.GRAD_NAMES)[worst]}) REF32 {r32:.3e} tolerance {tol:.3e}")
    assert tol <= F6_BOUND
    for name, d in zip(("out4",) + R.GRAD_NAMES, devs):
        assert d <= tol, (label, name, d, tol)
    return case


# ------------------------------------------------------------------------------------------------- 1. against fp64
@pytest.mark.parametrize("ci", range(len(R.CASES)))
def test_gradients_and_out4_against_fp64_on_two_steps(dev, ci):
    dims, mode, lr, level, rows, S, mixture = R.CASES[ci]
    cn = posthoc.compress(_net(dims, mode, lr, mixture, dev), level)
    x, y = _batch(mode, rows, dims, dev)
    step, _ = _step(cn, x, y, S)
    assert (cn.prior.mixture, cn.local_reparam) == (mixture, lr)
    c1 = _check_against_fp64(step, x, y, 0.3, f"case {ci} step 1")
    x2, y2 = _batch(mode, rows, dims, dev, seed=6)
    c2 = _check_against_fp64(step, x2, y2, 0.05, f"case {ci} step 2")    # the updated parameters, the NEXT S sample indices
    assert c2["first"] == c1["first"] + S and int(step.counter.item()) == 2 * S


@pytest.mark.parametrize("lr", [False, True])
def test_an_empty_row_among_full_ones_against_fp64(dev, lr):
    """F13's network: one row of layer 2 near zero, the lowest 0.5 % dropped -- an empty row between nearly full ones."""
    net = _net((119, 100, 1), "regression", lr, False, dev)
    with torch.no_grad():
        tiny = 1e-12 * (1 + torch.arange(100, device=dev, dtype=torch.float32))
        if lr:
            net.l2.weight_mu[:, 5] = tiny
        else:
            net.l2.weight_mu[5, :] = tiny
    cn = posthoc.compress(net, 0.005)
    rp = _np(cn._layers[1].row_ptr)
    assert rp[6] == rp[5] and (np.diff(rp) >= 95).sum() >= 98
    x, y = _batch("regression", 37, (119, 100, 1), dev)
    step, _ = _step(cn, x, y, 3)
    _check_against_fp64(step, x, y, 0.3, f"empty row lr={lr} step 1")
    _check_against_fp64(step, x, y, 0.3, f"empty row lr={lr} step 2")


def test_layers_without_a_survivor_are_legal(dev):
    """1-48-1 with parameter seed 2 at 98 %: layers 1 and 3 keep no weight at all (their kept biases, and layer 2, train on)."""
    cn = posthoc.compress(_net((1, 48, 1), "regression", False, False, dev, param_seed=2), .98)
    assert cn.nnz[0] == 0 and cn.nnz[2] == 0 and cn.nnz[1] > 0
    x, y = _batch("regression", 37, (1, 48, 1), dev)
    step, _ = _step(cn, x, y, 3)
    _check_against_fp64(step, x, y, 0.3, "empty layers step 1")
    _check_against_fp64(step, x, y, 0.3, "empty layers step 2")
    assert cn.nnz[0] == 0 and not cn._layers[0].mu_val.any()


# ------------------------------------------------------------------------------------------------- 2. level 0 against dense
def _keep_everything(net):
    """The CompressedNetwork of `net` with every weight and bias kept (a code image of ones at level 0)."""
    images = []
    for l in (net.l1, net.l2, net.l3):
        fout, fin = l.weight_mu.shape
        d = l.weight_mu.device
        images.append((fin, fout, torch.ones((-(-fout // 64) * 64, -(-fin // 32) * 32), dtype=torch.uint8, device=d),
                       torch.ones((1, -(-fout // 32) * 32), dtype=torch.uint8, device=d)))
    return posthoc.CompressedNetwork._build([net.l1, net.l2, net.l3], images, 0, False, net.mode, True)


@pytest.mark.parametrize("mixture", [False, True])
def test_level_0_agrees_with_the_dense_graphed_train_step(dev, mixture):
    dims, mode, rows, S, beta = (70, 130, 10), "classification", 37, 3, 0.3
    net = _net(dims, mode, False, mixture, dev)
    cn = _keep_everything(net)
    assert cn.nnz == (70 * 130, 130 * 130, 130 * 10)
    x, y = _batch(mode, rows, dims, dev)
    step, _ = _step(cn, x, y, S)
    case = _case_of(step, beta)
    tol = 4 * R.ref32_of(case)
    assert tol <= F6_BOUND
    s_out = _out4(step.step(x, y, beta))
    s_g = _grads(step)
    manual_seed(SEED, 0)                                                  # the same sample indices
    dense = GraphedTrainStep(net, FusedAdam(net.parameters(), lr=1e-3, capturable=True), x, y, S)
    d_out = _out4(dense.step(x, y, beta))
    d_g = [_np(g).copy() for g in dense.grad_views]
    assert R.rel_dev(s_out, d_out) <= tol, (s_out, d_out)
    for i, l in enumerate(case["layers"]):
        want = [d_g[4 * i][l["rows"], l["col"]], d_g[4 * i + 1][l["rows"], l["col"]], d_g[4 * i + 2], d_g[4 * i + 3]]
        for name, a, b in zip(R.GRAD_NAMES[4 * i:4 * i + 4], s_g[4 * i:4 * i + 4], want):
            print(f"level 0 mixture={mixture} {name}: sparse vs dense {R.rel_dev(a, b):.3e} (tolerance {tol:.3e})")
            assert R.rel_dev(a, b) <= tol, name


# ------------------------------------------------------------------------------------------------- 3. Adam, sigma
def _bits(t):
    return t.contiguous().view(torch.int32)


def test_adam_and_the_sigma_refresh_bit_for_bit(dev):
    dims, mode = (70, 130, 10), "classification"
    cn = posthoc.compress(_net(dims, mode, False, False, dev), .5)
    x, y = _batch(mode, 37, dims, dev)
    step, opt = _step(cn, x, y, 3, lr=2e-3)
    before = [p.detach().clone() for p in cn.parameters()]
    mc_before = cn.forward_mc(x, 2, seed=SEED, sample_offset=50).clone()  # the plan for (37 rows, 2 samples) exists before the step
    step.step(x, y, 0.3)
    grads = [g.clone() for g in step.grad_views]
    twins = [torch.nn.Parameter(b.clone()) for b in before]
    for t, g in zip(twins, grads):
        t.grad = g
    FusedAdam(twins, lr=2e-3, capturable=True).step()                    # eager (not captured), fed the step's own gradients
    for name, p, t in zip(R.GRAD_NAMES, cn.parameters(), twins):
        assert torch.equal(_bits(p.detach()), _bits(t.detach())), name
        assert not torch.equal(p.detach(), before[R.GRAD_NAMES.index(name)]), name
    for c, keep in zip(cn._layers, step.keep):
        assert torch.equal(_bits(c.sigma_val[:c.nnz]), _bits(ops.softplus(c.rho_val)[:c.nnz]))
        want = torch.where(keep.bool(), ops.softplus(c.b_rho), torch.zeros_like(c.b_rho))
        assert torch.equal(_bits(c.b_sigma), _bits(want))
    # the forward afterwards, layer by layer through the launch forward_mc makes, within the derived chain bound
    rs = np.random.RandomState(1)
    for c in cn._layers:
        n = c.nnz
        x_np = rs.uniform(-1, 1, (37, c.fin)).astype(np.float32)
        f = dict(dtype=torch.float32, device=dev)
        yv, dump, dump_b = torch.empty((1, 37, c.fout), **f), torch.empty((1, max(n, 1)), **f), torch.empty((1, c.fout), **f)
        ops.sparse_fwd(ops.sparse_fwd_args(row_ptr=c.row_ptr, col=c.col, mu_val=c.mu_val, sigma_val=c.sigma_val, b_mu=c.b_mu,
                                           b_sigma=c.b_sigma, x=torch.from_numpy(x_np).to(dev), y=yv, n_samples=1, rows=37,
                                           in_features=c.fin, out_features=c.fout, eps_mode=L.EPS_PHILOX, relu=False,
                                           layer_id=c.layer_id, seed=SEED, sample_offset=40, eps_dump=dump, eps_b_dump=dump_b))
        r = dict(row_ptr=_np(c.row_ptr), col=_np(c.col)[:n].view(np.uint16), mu_val=_np(c.mu_val)[:n], sigma_val=_np(c.sigma_val)[:n],
                 b_mu=_np(c.b_mu), b_sigma=_np(c.b_sigma), fin=c.fin)
        ref, w, b = sparse_layer_ref(r, x_np, (_np(dump)[0, :n], _np(dump_b)[0]))
        assert np.all(np.abs(_np(yv)[0].astype(np.float64) - ref) <= chain_bound_layer(x_np, r["row_ptr"], r["col"], w, b))
    # forward_mc itself, through the plan cached before the step: the whole network on the UPDATED parameters against the
    # fp64 restatement, epsilon being the dense map's at sample_offset + s (the device's bits, as tests/test_gpu_sparse.py takes it)
    mc = cn.forward_mc(x, 2, seed=SEED, sample_offset=50).clone()
    layers = []
    for c in cn._layers:
        n = c.nnz
        rp = _np(c.row_ptr)
        layers.append(dict(row_ptr=rp, col=_np(c.col)[:n].view(np.uint16), rows=np.repeat(np.arange(c.fout), np.diff(rp)),
                           mu_val=_np(c.mu_val)[:n], sigma_val=_np(ops.softplus(c.rho_val))[:n], b_mu=_np(c.b_mu),
                           b_sigma=_np(torch.where(c.b_sigma != 0, ops.softplus(c.b_rho), torch.zeros_like(c.b_rho))), fin=c.fin))
    for s_ in range(2):
        eps = []
        for c, l in zip(cn._layers, layers):
            ew = _np(ops.philox_normal(SEED, 4 * c.layer_id, 50 + s_, 1, c.fout, c.fin, dev))[0]
            eb = _np(ops.philox_normal(SEED, 4 * c.layer_id + 1, 50 + s_, 1, 1, c.fout, dev))[0, 0]
            eps.append((ew[l["rows"], l["col"].astype(np.int64)], eb))
        want = sparse_forward_ref(layers, _np(x), eps)
        err, scale = np.abs(_np(mc[s_]).astype(np.float64) - want).max(), np.abs(want).max()
        moved = np.abs(_np(mc_before[s_]).astype(np.float64) - want).max()
        print(f"forward_mc after the step, sample {s_}: err {err:.3e} scale {scale:.3e}; the logits before the step differ by {moved:.3e}")
        assert err <= FWD_TOL * scale
        assert moved > 10 * FWD_TOL * scale                               # stale parameters would not have passed


def test_relu_in_the_backward_equals_a_mask_applied_beforehand(dev):
    """bnn_sparse_bwd with relu = 1 (gz = gy * (y > 0), its own launch) against the same call fed the masked gy: the same bits."""
    cn = posthoc.compress(_net((70, 130, 10), "classification", False, True, dev), .5)
    c, S, rows = cn._layers[1], 2, 37
    g = torch.Generator(device="cpu").manual_seed(3)
    f = dict(dtype=torch.float32)
    xin = torch.rand((S, c.fin, rows), generator=g, **f).to(dev)
    yv = (torch.rand((S, c.fout, rows), generator=g, **f) - 0.4).clamp_min(0).to(dev)
    gy = torch.randn((S, c.fout, rows), generator=g, **f).to(dev)
    from bnn_hip.sparse_train import csc_view
    cp, rw, pm = csc_view(c.row_ptr, c.col, c.nnz, c.fin)
    keep = (c.b_sigma != 0).to(torch.uint8)
    outs = []
    for relu, gin, yy in ((True, gy, yv), (False, gy * (yv > 0), None)):
        o = [torch.full((max(c.nnz, 1),), float("nan"), device=dev) for _ in range(2)] + \
            [torch.full((c.fout,), float("nan"), device=dev) for _ in range(2)] + [torch.full((S, c.fin, rows), float("nan"), device=dev)]
        ops.sparse_bwd(ops.sparse_bwd_args(
            row_ptr=c.row_ptr, col=c.col, mu_val=c.mu_val, rho_val=c.rho_val, b_mu=c.b_mu, b_rho=c.b_rho, b_keep=keep, x=xin,
            gy=gin.contiguous(), y=yy, g_mu_val=o[0], g_rho_val=o[1], g_b_mu=o[2], g_b_rho=o[3], g_x=o[4],
            workspace=ops.sparse_bwd_workspace(S, rows, c.fout, dev), n_samples=S, rows=rows, in_features=c.fin,
            out_features=c.fout, nnz=c.nnz, prior=cn.prior, relu=relu, gy_row_major=False, x_per_sample=1, gx_relu_mask=True,
            layer_id=c.layer_id, seed=SEED, sample_offset=9, col_ptr=cp, row=rw, perm=pm))
        outs.append(o)
    for a, b in zip(*outs):
        assert torch.isfinite(a).all()                                    # every element was written
        assert torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------- 4. the pattern is fixed
def test_the_pattern_stays_fixed_over_five_steps(dev):
    dims, mode = (70, 130, 10), "classification"
    cn = posthoc.compress(_net(dims, mode, True, False, dev), .98)
    x, y = _batch(mode, 37, dims, dev)
    pattern = [(c.row_ptr.clone(), c.col.clone(), c.nnz) for c in cn._layers]
    pruned_bias = [(c.b_sigma == 0).clone() for c in cn._layers]
    assert any(bool(m.any()) for m in pruned_bias) and any(bool((~m).any()) for m in pruned_bias)
    zero = {k: (v == 0) for k, v in cn.to_dense().items()}
    step, _ = _step(cn, x, y, 2, lr=1e-2)
    for _ in range(5):
        step.step(x, y, 0.3)
    for c, (rp, col, nnz), m in zip(cn._layers, pattern, pruned_bias):
        assert torch.equal(c.row_ptr, rp) and torch.equal(c.col, col) and c.nnz == nnz
        assert not c.b_mu[m].any() and not c.b_rho[m].any() and not c.b_sigma[m].any()       # every pruned bias is still 0
    for k, v in cn.to_dense().items():
        assert torch.equal(v == 0, zero[k]), k                                               # zero exactly where it was


# ------------------------------------------------------------------------------------------------- 5. reproducible
def _state_of(cn, opt, step=None):
    out = [p.detach().clone() for p in cn.parameters()] + [t.clone() for c in cn._layers for t in (c.sigma_val, c.b_sigma)]
    for p in cn.parameters():
        st = opt.state.get(p, {})
        out += [st[k].clone() for k in ("exp_avg", "exp_avg_sq") if k in st]
    return out


def test_two_objects_replay_and_eager_launches_give_the_same_bits(dev):
    dims, mode = (70, 130, 10), "classification"
    net = _net(dims, mode, False, True, dev)
    x, y = _batch(mode, 300, dims, dev)
    cns = [posthoc.compress(net, .5) for _ in range(3)]
    before = [p.detach().clone() for p in cns[0].parameters()]
    built = [_step(cn, x, y, 3) for cn in cns]
    # building a step object leaves the parameters, moments, step word and counter as they were
    step0, opt0 = built[0]
    for p, b in zip(cns[0].parameters(), before):
        assert torch.equal(_bits(p.detach()), _bits(b))
    for p in cns[0].parameters():
        st = opt0.state.get(p, {})
        assert all(not st[k].any() for k in ("exp_avg", "exp_avg_sq") if k in st)
    assert opt0.device_step() == 0 and int(step0.counter.item()) == 0 and state.counter == 0
    outs = []
    for k, (step, opt) in enumerate(built):
        manual_seed(SEED, 0)                                              # every object draws the sample indices 0 .. 8
        for j in range(3):
            if k < 2:
                o = step.step(x, y, 0.1 * (j + 1))                        # graph replays
            else:
                step.x.copy_(x)
                step.y.copy_(y)
                step.beta.fill_(0.1 * (j + 1))
                o = step.eager()                                          # the same launches issued one by one
        torch.cuda.synchronize()
        outs.append((_state_of(step.cn, opt), [t.clone() for t in o], step.bucket.clone()))
    for other in outs[1:]:
        for group_a, group_b in zip(outs[0], other):
            for a, b in zip(group_a, group_b) if isinstance(group_a, list) else ((group_a, group_b),):
                assert torch.equal(_bits(a), _bits(b))
    assert not torch.equal(outs[0][0][0], before[0])


# ------------------------------------------------------------------------------------------------- 6. EpochRunner
def test_an_epoch_runner_equals_a_host_loop_of_steps(dev):
    dims, mode, B, M = (70, 130, 10), "classification", 32, 4
    net = _net(dims, mode, False, False, dev)
    X, Y = _batch(mode, B * M, dims, dev, seed=8)
    results = []
    for runner in (True, False):
        cn = posthoc.compress(net, .5)
        step, opt = _step(cn, X[:B], Y[:B], 2)
        loader = DeviceLoader(DeviceDataset(X, Y), B, shuffle=False)
        if runner:
            hist = EpochRunner(step, loader).run_epoch()
        else:
            betas = beta_table(M)
            hist = torch.stack([torch.cat([o.reshape(1) for o in step.step(X[j * B:(j + 1) * B], Y[j * B:(j + 1) * B], float(betas[j]))])
                                for j in range(M)])
        torch.cuda.synchronize()
        results.append((hist.clone(), _state_of(cn, opt)))
    assert tuple(results[0][0].shape) == (M, 4)
    assert torch.equal(_bits(results[0][0]), _bits(results[1][0]))
    for a, b in zip(results[0][1], results[1][1]):
        assert torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------- 7. learns
def test_fine_tuning_a_pruned_network_lowers_the_loss(dev):
    dims, mode, B = (70, 130, 10), "classification", 128
    rs = np.random.RandomState(12)
    X = rs.uniform(0, 1, (512, 70)).astype(np.float32)
    Yl = (X @ rs.standard_normal((70, 10))).argmax(1).astype(np.int64)                      # labels a network can learn
    X, Yl = torch.from_numpy(X).to(dev), torch.from_numpy(Yl).to(dev)
    cn = posthoc.compress(_net(dims, mode, False, False, dev), .75)
    nnz = cn.nnz
    step, _ = _step(cn, X[:B], Yl[:B], 2, lr=1e-3)
    losses = []
    for j in range(200):
        k = (j % 4) * B
        losses.append(step.step(X[k:k + B], Yl[k:k + B], 0.25)[0].clone())
    losses = torch.cat(losses).cpu().numpy()
    print(f"fine-tuning at 75 %: mean loss of the first 20 steps {losses[:20].mean():.2f}, of the last 20 {losses[-20:].mean():.2f}")
    assert np.isfinite(losses).all() and losses[-20:].mean() < losses[:20].mean()
    assert cn.nnz == nnz
