"""GPU checks of the Flipout estimator (csrc/flipout.hip, bnn_hip.flipout; include/bnn_hip.h F16) against the numpy fp64
restatement tests/flipout_ref.py: the sign stream bit for bit, the layer forward inside the rigorous fp32 summation bound in
f32 and bf16 math, on-chip epsilon = injected epsilon bit for bit, the ELBO terms, every gradient, the bf16 network, the
captured training step against the eager loop bit for bit, and the refusals."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bnn_hip
import flipout_ref as R
from bnn_hip import _lib as L
from bnn_hip import ops
from bnn_hip.ops import BnnHipError, PriorSpec

SEED = 2026
F32_RTOL = 2e-5
# bf16 math (operands and hidden activations rounded to bf16) against the fp64 restatement on UN-rounded operands, 784-64-64-10,
# batch 32, S = 4: max |logit - ref| / max |ref| measured on an MI355X is 5.41e-3 at D = 1 and 5.90e-3 at D = 4; the bound is
# 3 x the larger, as BF16_LOGIT_TOL of tests/test_gpu_parity.py was set.
BF16_FLIPOUT_LOGIT_TOL = 1.8e-2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _f32_math():
    bnn_hip.set_math("f32")
    yield
    bnn_hip.set_math("bf16")
    bnn_hip.shard_samples(False)


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N_(t):
    return t.detach().cpu().numpy()


def bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).float().numpy()


class Replay:
    def __init__(self, arrays):
        self.q = [torch.from_numpy(np.ascontiguousarray(a)) for a in arrays]

    def sample(self, size):
        t = self.q.pop(0)
        assert tuple(t.shape) == tuple(size)
        return t


# ---------------------------------------------------------------------------------------------- signs
@pytest.mark.parametrize("rows,cols", [(19, 37), (3, 130), (131, 21)])
def test_signs_equal_the_restatement_bit_for_bit(dev, rows, cols):
    for kind in (0, 1):
        for off in (0, 7):
            got = N_(ops.flipout_signs(SEED, 2, kind, 5, 3, rows, cols, dev, row_offset=off))
            want = R.sign_block(SEED, 2, kind, 5, 3, rows, cols, row_offset=off)
            assert got.dtype == np.int8 and (got == want).all(), (kind, off)
    cut = rows // 2 + 1
    whole = ops.flipout_signs(SEED, 1, 0, 9, 3, rows, cols, dev)
    a = ops.flipout_signs(SEED, 1, 0, 9, 3, cut, cols, dev)
    b = ops.flipout_signs(SEED, 1, 0, 9, 3, rows - cut, cols, dev, row_offset=cut)
    assert torch.equal(whole, torch.cat([a, b], dim=1))


# ---------------------------------------------------------------------------------------------- layer forward
def _layer(seed, K, N, B, S, D, per_sample):
    rng = np.random.default_rng(seed)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return dict(x=f(rng.standard_normal((S, B, K) if per_sample else (B, K))), mu=f(rng.uniform(-0.3, 0.3, (N, K))),
                rho=f(rng.uniform(-4.0, -1.0, (N, K))), bm=f(rng.uniform(-0.3, 0.3, N)), br=f(rng.uniform(-4.0, -1.0, N)),
                ew=f(rng.standard_normal((D, N, K))), eb=f(rng.standard_normal((D, N))))


def _run_layer(dev, c, S, D, relu, math_mode, layer_id=1, first=5, eps_mode=L.EPS_MEMORY, want_stats=False, prior=PriorSpec(False, 1.0)):
    p = [T(c[k], dev) for k in ("mu", "rho", "bm", "br")]
    prep = ops.flipout_prepare(*p, n_samples=S, n_draws=D, prior=prior, math_mode=math_mode, eps_mode=eps_mode,
                               eps_w=T(c["ew"], dev) if eps_mode == L.EPS_MEMORY else None,
                               eps_b=T(c["eb"], dev) if eps_mode == L.EPS_MEMORY else None, seed=SEED, layer_id=layer_id,
                               sample_offset=first, want_stats=want_stats, want_eps=True)
    y = ops.flipout_fwd(T(c["x"], dev), prep, p[0], p[2], n_samples=S, n_draws=D, math_mode=math_mode, relu=relu, eps_mode=eps_mode,
                        seed=SEED, layer_id=layer_id, sample_offset=first)
    return prep, y


def _check_forward(dev, c, K, N, B, S, D, relu, math_mode):
    prep, y = _run_layer(dev, c, S, D, relu, math_mode)
    sw = N_(ops.softplus(T(c["rho"], dev)))
    sb = N_(ops.softplus(T(c["br"], dev)))
    delta = sw[None] * c["ew"]                                          # fp32 product, rounded once: fl32(sigma * eps)
    assert delta.dtype == np.float32 and (N_(prep["delta"]) == delta).all()
    b = c["bm"].astype(np.float64) + sb.astype(np.float64) * c["eb"].astype(np.float64)
    assert np.abs(N_(prep["b_draw"]) - b).max() <= 2.0 ** -23 * np.abs(b).max()
    r = R.sign_block(SEED, 1, 0, 5, S, B, K)
    s = R.sign_block(SEED, 1, 1, 5, S, B, N)
    x, mu, dl = c["x"], c["mu"], delta
    if math_mode == L.MATH_BF16:
        x, mu, dl = bf16_round(x), bf16_round(mu), bf16_round(delta)
        assert (prep["delta_bf16"].float().cpu().numpy() == dl).all() and (prep["mu_bf16"].float().cpu().numpy() == mu).all()
    y64, pre = R.forward(x, mu, dl, b, r, s, relu)
    bnd = R.bound(x, mu, dl, b, S, K)
    got = N_(y).astype(np.float64)
    assert got.shape == (S, B, N)
    err = np.abs(got - y64)
    print(f"flipout fwd K={K} N={N} B={B} S={S} D={D} relu={relu} math={math_mode}: max err/bound = {(err / bnd).max():.3f}")
    if relu:
        sure = np.abs(pre) > bnd
        assert (err[sure] <= bnd[sure]).all()
        assert (got[~sure] >= 0).all() and (got[~sure] <= np.abs(pre[~sure]) + bnd[~sure]).all()
    else:
        assert (err <= bnd).all()


SHAPES = [(37, 21, 19), (130, 131, 131), (64, 1, 1), (33, 10, 128)]


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("D", [1, 3, 6])
@pytest.mark.parametrize("K,N,B", SHAPES)
def test_layer_forward_f32_within_the_summation_bound(dev, K, N, B, D, relu):
    c = _layer(K * 1000 + N, K, N, B, 6, D, per_sample=(D == 3))
    _check_forward(dev, c, K, N, B, 6, D, relu, L.MATH_F32)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("D", [1, 3, 6])
@pytest.mark.parametrize("K,N,B", SHAPES)
def test_layer_forward_bf16_within_the_summation_bound(dev, K, N, B, D, relu):
    c = _layer(K * 1000 + N + 1, K, N, B, 6, D, per_sample=(D == 3))
    _check_forward(dev, c, K, N, B, 6, D, relu, L.MATH_BF16)


def test_mean_path(dev):
    c = _layer(3, 37, 21, 19, 1, 1, False)
    y = ops.flipout_fwd(T(c["x"], dev), None, T(c["mu"], dev), T(c["bm"], dev), n_samples=1, n_draws=1, math_mode=L.MATH_F32, relu=False,
                        eps_mode=L.EPS_ZERO)
    want = c["x"].astype(np.float64) @ c["mu"].astype(np.float64).T + c["bm"]
    bnd = (37 + 8) * 2.0 ** -24 * (np.abs(c["x"]).astype(np.float64) @ np.abs(c["mu"]).astype(np.float64).T + np.abs(c["bm"]))
    assert (np.abs(N_(y)[0] - want) <= bnd).all()


# ---------------------------------------------------------------------------------------------- Philox = memory
def test_on_chip_epsilon_equals_injected_epsilon_bit_for_bit(dev):
    K, N, B, S, D, lid, first = 37, 21, 19, 4, 2, 1, 40
    c = _layer(9, K, N, B, S, D, False)
    prep_p, y_p = _run_layer(dev, c, S, D, True, L.MATH_F32, layer_id=lid, first=first, eps_mode=L.EPS_PHILOX)
    ew = torch.cat([ops.philox_normal(SEED, 4 * lid, first + d * (S // D), 1, N, K, dev) for d in range(D)])
    eb = torch.cat([ops.philox_normal(SEED, 4 * lid + 1, first + d * (S // D), 1, 1, N, dev) for d in range(D)]).reshape(D, N)
    assert torch.equal(prep_p["eps_w"], ew) and torch.equal(prep_p["eps_b"], eb)
    c2 = dict(c, ew=N_(ew), eb=N_(eb))
    prep_m, y_m = _run_layer(dev, c2, S, D, True, L.MATH_F32, layer_id=lid, first=first, eps_mode=L.EPS_MEMORY)
    assert torch.equal(y_p, y_m) and torch.equal(prep_p["delta"], prep_m["delta"]) and torch.equal(prep_p["b_draw"], prep_m["b_draw"])
    # S = 4 as 2 + 2 with the sample offset advanced
    halves = [_run_layer(dev, c, 2, 1, True, L.MATH_F32, layer_id=lid, first=first + 2 * h, eps_mode=L.EPS_PHILOX)[1] for h in range(2)]
    assert torch.equal(torch.cat(halves), y_p)
    # D = S: the epsilon BayesianLinear draws for the same seed, layer and sample index
    prep_s, _ = _run_layer(dev, c, S, S, True, L.MATH_F32, layer_id=lid, first=first, eps_mode=L.EPS_PHILOX)
    p = [T(c[k], dev) for k in ("mu", "rho", "bm", "br")]
    bbb = ops.bbb_linear_fwd(T(c["x"], dev), *p, n_samples=S, prior=PriorSpec(False, 1.0), math_mode=L.MATH_F32, relu=True,
                             y_dtype=torch.float32, eps_mode=L.EPS_PHILOX, seed=SEED, layer_id=lid, sample_offset=first,
                             want_stats=False, dump_eps=True)
    assert torch.equal(prep_s["eps_w"], bbb["eps_w"]) and torch.equal(prep_s["eps_b"], bbb["eps_b"])


# ---------------------------------------------------------------------------------------------- ELBO terms
@pytest.mark.parametrize("prior", [("gauss", 0.7), ("mixture", 0.5, 1.0, math.exp(-6.0))])
@pytest.mark.parametrize("K,N,D", [(37, 21, 3), (130, 131, 2), (1, 33, 1)])
def test_elbo_terms_against_fp64(dev, prior, K, N, D):
    c = _layer(77, K, N, 4, D, D, False)
    spec = PriorSpec(False, prior[1]) if prior[0] == "gauss" else PriorSpec(True, 1.0, prior[1], prior[2], prior[3])
    prep, _ = _run_layer(dev, c, D, D, False, L.MATH_F32, want_stats=True, prior=spec)
    lp, lq = R.elbo_terms(c["mu"], c["rho"], c["bm"], c["br"], c["ew"], c["eb"], prior)
    np.testing.assert_allclose(N_(prep["log_prior"]), lp, rtol=F32_RTOL)
    np.testing.assert_allclose(N_(prep["log_q"]), lq, rtol=F32_RTOL)


# ---------------------------------------------------------------------------------------------- networks
def _mp(dims, mode, mixture=True):
    return dict(input_shape=dims[0], classes=dims[2], batch_size=19, hidden_units=dims[1], mode=mode, mu_init=[-0.2, 0.2],
                rho_init=[-5, -4], prior_init=[0.5, 0, -6] if mixture else [1.0], mixture_prior=mixture, local_reparam=False)


def _net(dev, dims, mode, seed, base_draws=1, mixture=True):
    import networks
    torch.manual_seed(seed)
    return networks.FlipoutNetwork(_mp(dims, mode, mixture), base_draws=base_draws).to(dev).train()


def _params(net):
    return [tuple(N_(t) for t in (l.weight_mu, l.weight_rho, l.bias_mu, l.bias_rho)) for l in (net.l1, net.l2, net.l3)]


def _eps(net, D, seed):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((D,) + tuple(l.weight_mu.shape)).astype(np.float32),
             rng.standard_normal((D,) + tuple(l.bias_mu.shape)).astype(np.float32)) for l in (net.l1, net.l2, net.l3)]


def _inject(net, eps, D):
    layers = (net.l1, net.l2, net.l3)
    for i, l in enumerate(layers):
        l.weight.normal = Replay([eps[i][0][d] for d in range(D)])
        l.bias.normal = Replay([eps[i][1][d] for d in range(D)])


def _data(dims, mode, B, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, dims[0])).astype(np.float32)
    y = rng.integers(0, dims[2], B) if mode == "classification" else rng.standard_normal((B, dims[2])).astype(np.float32)
    return x, y


PRIOR_MIX = ("mixture", 0.5, 1.0, math.exp(-6.0))


@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("dims,mode", [((37, 21, 5), "classification"), ((1, 33, 1), "regression")])
def test_network_gradients_against_the_restatement(dev, dims, mode, D):
    S, B, beta, sigma = 4, 19, 0.25, 0.5 if mode == "regression" else 1.0
    net = _net(dev, dims, mode, 3)
    x, y = _data(dims, mode, B, 4)
    eps = _eps(net, D, 5)
    ref = R.network(_params(net), x, eps, bnn_hip.runtime.state.seed, 0, S, D, PRIOR_MIX, mode, y, beta, sigma)

    def run():
        _inject(net, eps, D)
        net.zero_grad()
        xt = T(x, dev).requires_grad_(True)
        out = net.sample_elbo(xt, T(y, dev), beta, S, sigma, base_draws=D)
        out[0].backward()
        return out, [p.grad.clone() for p in net.parameters()], xt.grad.clone()
    out, grads, gx = run()
    for got, want in zip(out, (ref["loss"], ref["log_prior"], ref["log_q"], ref["nll"])):
        np.testing.assert_allclose(N_(got).reshape(-1)[0], want, rtol=1e-4)
    flat = [g for layer in ref["grads"] for g in layer]
    for (name, _), got, want in zip(net.named_parameters(), grads, flat):
        np.testing.assert_allclose(N_(got), want, rtol=2e-4, atol=2e-5 * np.abs(want).max(), err_msg=name)
    np.testing.assert_allclose(N_(gx), ref["g_x"], rtol=2e-4, atol=2e-5 * np.abs(ref["g_x"]).max())
    out2, grads2, gx2 = run()                                           # a repeated step from one state: the same bits
    assert all(torch.equal(a, b) for a, b in zip(grads, grads2)) and torch.equal(gx, gx2)
    assert all(torch.equal(a, b) for a, b in zip(out, out2))


@pytest.mark.parametrize("D", [1, 4])
def test_network_logits_bf16(dev, D):
    dims, B, S = (784, 64, 10), 32, 4
    bnn_hip.set_math("bf16")
    net = _net(dev, dims, "classification", 6)
    x, _ = _data(dims, "classification", B, 7)
    x = np.abs(x) / 3.0
    eps = _eps(net, D, 8)
    _inject(net, eps, D)
    lg = N_(net.forward_mc(T(x, dev), S, base_draws=D)).astype(np.float64)
    ref = R.network(_params(net), x, eps, bnn_hip.runtime.state.seed, 0, S, D, PRIOR_MIX, "classification", np.zeros(B, np.int64), 0.0)
    err = np.abs(lg - ref["logits"]).max() / np.abs(ref["logits"]).max()
    print(f"flipout bf16 logits D={D}: max |err| / max |logit| = {err:.3e}")
    assert err <= BF16_FLIPOUT_LOGIT_TOL


def test_network_surface(dev):
    """forward / forward_mc / predict_mc / predictive / score run, draw fresh noise per call, and the view shares storage."""
    import networks
    torch.manual_seed(1)
    bbb = networks.BayesianNetwork(_mp((37, 21, 5), "classification")).to(dev)
    net = bbb.flipout()
    assert net.l1.weight_mu.data_ptr() == bbb.l1.weight_mu.data_ptr()
    x, y = _data((37, 21, 5), "classification", 19, 2)
    xt, yt = T(x, dev), T(y, dev)
    net.eval()
    bnn_hip.manual_seed(5, counter=100)
    mean = net(xt)
    assert torch.equal(mean, net(xt)) and bnn_hip.runtime.state.counter == 100
    a, b = net.forward_mc(xt, 4), net.forward_mc(xt, 4)
    assert a.shape == (4, 19, 5) and not torch.equal(a, b) and bnn_hip.runtime.state.counter == 108
    assert not torch.equal(a[0], a[1])                                   # one base draw, different signs per sample
    bnn_hip.manual_seed(5, counter=100)
    assert torch.equal(net.forward_mc(xt, 4), a)
    preds, probs = net.predict_mc(xt, 4, base_draws=4)
    assert preds.shape == (19,) and torch.allclose(probs.sum(1), torch.ones(19, device=dev), atol=1e-5)
    p = net.predictive(xt, 8, base_draws=2)
    assert p.probs.shape == (19, 5) and bool((p.mutual_information >= 0).all())
    sc = net.score(xt, yt, 8).read()
    assert math.isfinite(sc.lpd) and sc.n == 19
    assert net.take_samples(3) == bnn_hip.runtime.state.counter - 3


# ---------------------------------------------------------------------------------------------- the captured step
def _beta(M, i):
    return 2 ** (M - (i + 1)) / (2 ** M - 1)


def test_graphed_train_step_equals_eager_steps_bit_for_bit(dev):
    from bnn_hip.optim import FusedAdam
    dims, B, S, M = (37, 21, 5), 19, 2, 3
    net_a, net_b = _net(dev, dims, "classification", 11), _net(dev, dims, "classification", 12)
    net_b.load_state_dict(net_a.state_dict())
    data = [_data(dims, "classification", B, 20 + i) for i in range(M)]
    xs, ys = [T(d[0], dev) for d in data], [T(d[1], dev) for d in data]
    oa = FusedAdam(net_a.parameters(), lr=1e-3, capturable=True)
    ob = FusedAdam(net_b.parameters(), lr=1e-3, capturable=True)
    bnn_hip.manual_seed(99, counter=500)
    before = {k: v.clone() for k, v in net_b.state_dict().items()}
    g = net_b.graphed_train_step(ob, xs[0], ys[0], S, base_draws=1)
    for k, v in net_b.state_dict().items():
        assert torch.equal(v, before[k]), k
    for p in net_b.parameters():
        assert not bool(ob.state[p]["exp_avg"].any()) and not bool(ob.state[p]["exp_avg_sq"].any())
    assert ob.device_step() == 0 and int(g.counter.item()) == 0 and bnn_hip.runtime.state.counter == 500
    outs = [[o.clone() for o in g.step(xs[i], ys[i], _beta(M, i))] for i in range(M)]
    assert ob.device_step() == M and int(g.counter.item()) == M * S and bnn_hip.runtime.state.counter == 500 + M * S
    bnn_hip.manual_seed(99, counter=500)
    for i in range(M):
        oa.zero_grad()
        out = net_a.sample_elbo(xs[i], ys[i], _beta(M, i), S, base_draws=1)
        out[0].backward()
        oa.step()
        for got, want in zip(outs[i], out):
            assert torch.equal(got.reshape(-1), want.detach().reshape(-1)), i
    for (k, a), (_, b) in zip(net_a.state_dict().items(), net_b.state_dict().items()):
        assert torch.equal(a, b), k


def test_epoch_runner_drives_the_flipout_step(dev):
    from bnn_hip import epoch
    from bnn_hip.optim import FusedAdam
    dims, B, M, S = (37, 21, 5), 19, 4, 2
    X, Y = _data(dims, "classification", B * M + 3, 31)
    order = torch.randperm(B * M + 3, generator=torch.Generator().manual_seed(13))

    def run(runner):
        bnn_hip.manual_seed(SEED, counter=1000)
        net = _net(dev, dims, "classification", 21)
        opt = FusedAdam(net.parameters(), lr=1e-3, capturable=True)
        ld = epoch.DeviceLoader(epoch.DeviceDataset(X, Y, device=dev), B, seed=77)
        step = net.graphed_train_step(opt, *ld.example(), S)
        if runner:
            hist = epoch.EpochRunner(step, ld).run_epoch(order).clone()
        else:
            Xd, Yd = T(X, dev), T(Y, dev)
            rows = []
            for j in range(M):
                idx = order[j * B:(j + 1) * B].to(dev)
                rows.append(torch.cat([o.reshape(1) for o in step.step(Xd[idx], Yd[idx], _beta(M, j))]))
            hist = torch.stack(rows)
        torch.cuda.synchronize()
        return hist, [p.detach().clone() for p in net.parameters()], bnn_hip.runtime.state.counter
    h0, p0, c0 = run(False)
    h1, p1, c1 = run(True)
    assert c0 == c1 == 1000 + M * S and h1.shape == (M, 4)
    assert torch.equal(h0, h1) and all(torch.equal(a, b) for a, b in zip(p0, p1))


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals(dev):
    import networks
    from bnn_hip import active, epoch
    from bnn_hip.optim import FusedAdam
    net = _net(dev, (37, 21, 5), "classification", 1)
    x, y = _data((37, 21, 5), "classification", 19, 2)
    xt, yt = T(x, dev), T(y, dev)
    bnn_hip.set_math("bf16x3")
    with pytest.raises(BnnHipError, match="bf16x3"):
        net.forward_mc(xt, 2)
    with pytest.raises(BnnHipError, match="bf16x3"):
        net.graphed_train_step(FusedAdam(net.parameters(), capturable=True), xt, yt, 2)
    bnn_hip.set_math("f32")
    bnn_hip.shard_samples(True)
    with pytest.raises(BnnHipError, match="shard"):
        net.forward_mc(xt, 2)
    bnn_hip.shard_samples(False)
    with L.recording():
        with pytest.raises(BnnHipError, match="recorded"):
            net.forward_mc(xt, 2)
    with pytest.raises(BnnHipError, match="stacked"):
        net.predictive(xt, 2, stacked=True)
    with pytest.raises(BnnHipError, match="divide"):
        net.forward_mc(xt, 4, base_draws=3)
    with pytest.raises(BnnHipError, match="local_reparam"):
        networks.BayesianNetwork(dict(_mp((37, 21, 5), "classification", False), local_reparam=True)).flipout()
    stub = _net(dev, (37, 21, 5), "classification", 1)
    _inject(stub, _eps(stub, 1, 3), 1)
    with pytest.raises(BnnHipError, match="captured"):
        stub.graphed_train_step(FusedAdam(stub.parameters(), capturable=True), xt, yt, 2)
    pool = active.ActivePool(epoch.DeviceDataset(x, y, device=dev), [0, 1])
    with pytest.raises(BnnHipError, match="per row"):
        pool.joint_probs(net, 4)
