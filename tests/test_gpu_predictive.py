"""MC predictive summaries on the device (bnn_mc_predictive, net.predictive / net.predictive_graph): the kernel against a
float64 numpy restatement, the end-to-end path against the reference's loops on injected epsilon, and the replayable
evaluation against the eager one at the same Philox sample indices."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bnn_hip
from bnn_hip import ops, synth
from oracle import bnn_oracle as O


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _f32_math():
    bnn_hip.set_math("f32")
    yield
    bnn_hip.set_math("bf16")


class Replay:
    def __init__(self, arrays):
        self.q = [torch.from_numpy(np.ascontiguousarray(a)) for a in arrays]

    def sample(self, size):
        t = self.q.pop(0)
        assert tuple(t.shape) == tuple(size)
        return t


def build_net(dev, lr, dims, mode, B=128):
    import networks
    mp = dict(input_shape=dims[0], classes=dims[2], batch_size=B, hidden_units=dims[1], mode=mode, mu_init=[-0.2, 0.2],
              rho_init=[-5, -4], prior_init=[1.0], mixture_prior=False, local_reparam=lr)
    net = networks.BayesianNetwork(mp)
    sd = synth.synth_state_dict(dims[0], dims[1], dims[2], lr)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net.to(dev).eval(), sd


def install_eps(net, B, S, lr):
    shapes = []
    for l in (net.l1, net.l2, net.l3):
        shapes += [(B, l.weight_mu.shape[1]) if lr else tuple(l.weight_mu.shape), tuple(l.bias_mu.shape)]
    per = [synth.synth_eps(shapes, s) for s in range(S)]
    for li, l in enumerate((net.l1, net.l2, net.l3)):
        if lr:
            l.normal = Replay([a for s in range(S) for a in (per[s][2 * li], per[s][2 * li + 1])])
        else:
            l.weight.normal = Replay([per[s][2 * li] for s in range(S)])
            l.bias.normal = Replay([per[s][2 * li + 1] for s in range(S)])
    return per


def np_classification(lg):
    """float64 restatement over logits [G, S, B, C]: (probs, predictive entropy, expected entropy, mutual information)."""
    lg = np.asarray(lg, np.float64)
    m = lg.max(-1, keepdims=True)
    e = np.exp(lg - m)
    p = e / e.sum(-1, keepdims=True)
    probs = p.mean(1)
    h = (np.log(e.sum(-1)) + m[..., 0]) - (p * lg).sum(-1)
    ee = h.mean(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        pe = -np.where(probs > 0, probs * np.log(probs), 0.0).sum(-1)
    return probs, pe, ee, np.maximum(pe - ee, 0.0)


def check_preds(preds, probs_ref):
    """preds exact, except on rows whose top-2 mean probabilities are within 1e-6."""
    top2 = np.sort(probs_ref, -1)[..., -2:]
    clear = (top2[..., 1] - top2[..., 0]) > 1e-6
    assert np.array_equal(preds[clear], probs_ref.argmax(-1)[clear])


CLASS_SHAPES = [(1, 10, 128, 10), (1, 1, 128, 10), (1, 64, 7, 3), (1, 5, 33, 100), (1, 257, 4, 2), (3, 10, 128, 10)]


@pytest.mark.parametrize("shape", CLASS_SHAPES)
def test_classification_kernel_matches_float64(dev, shape):
    G, S, B, C = shape
    rng = np.random.default_rng(G * 1000 + S * 7 + C)
    lg = (rng.standard_normal((G, S, B, C)) * 3).astype(np.float32)
    lg[:, :, 0] = rng.choice([-80.0, 80.0], size=(G, S, C)).astype(np.float32)     # saturated rows: p = 0 / 1 classes
    lg[:, :, 1, :2] = lg[:, :, 1].max(-1, keepdims=True) + 1.0                      # exact top-2 tie in every sample
    if B > 2:
        lg[:, :, 2, 1:] = -80.0                                                     # one class takes (almost) everything
        lg[:, :, 2, 0] = 80.0
    out = ops.mc_predictive(torch.from_numpy(lg).reshape(G * S, B, C).to(dev), "classification", groups=G)
    torch.cuda.synchronize()
    probs, pe, ee, mi = np_classification(lg)
    np.testing.assert_allclose(out.probs.cpu().numpy(), probs, rtol=0, atol=1e-6)
    np.testing.assert_allclose(out.predictive_entropy.cpu().numpy(), pe, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(out.expected_entropy.cpu().numpy(), ee, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(out.mutual_information.cpu().numpy(), mi, rtol=0, atol=2e-5)
    assert float(out.mutual_information.min()) >= 0.0
    preds = out.preds.cpu().numpy()
    check_preds(preds, probs)
    assert (preds[:, 1] == 0).all()                                                 # ties go to the lowest index
    assert tuple(out.probs.shape) == (G, B, C) and tuple(out.preds.shape) == (G, B)


LEVELS = [0.0, 0.25, 0.5, 0.75, 1.0, 0.1, 0.9, 1.0 / 3.0]


@pytest.mark.parametrize("S", [1, 2, 10, 1000, 1024])
def test_regression_kernel_matches_numpy(dev, S):
    G, B, C = 2, 37, 3
    rng = np.random.default_rng(S)
    y = (rng.standard_normal((G, S, B, C)) * 2 + 5).astype(np.float32)
    y[:, :, 3] = np.round(y[:, :, 3])                                               # ties
    y[:, :, 4, 0] = 1.25                                                            # a constant column
    if S > 3:
        y[1, 3, 5, 1] = np.nan                                                      # one NaN column
    out = ops.mc_predictive(torch.from_numpy(y).reshape(G * S, B, C).to(dev), "regression", groups=G, sigma=0.1,
                            quantiles=LEVELS)
    torch.cuda.synchronize()
    yd = y.astype(np.float64)
    np.testing.assert_allclose(out.mean.cpu().numpy(), yd.mean(1), rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(out.variance.cpu().numpy(), yd.var(1), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(out.predictive_variance.cpu().numpy(), yd.var(1) + 0.01, rtol=1e-5, atol=1e-6)
    want = np.stack([np.percentile(y, 100 * q, axis=1) for q in LEVELS])             # [Q, G, B, C]
    got = out.quantiles.cpu().numpy()
    assert got.shape == (len(LEVELS), G, B, C)
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=0)
    if S > 3:
        assert np.isnan(got[:, 1, 5, 1]).all() and not np.isnan(np.delete(got.reshape(len(LEVELS), -1), 1 * B * C + 5 * C + 1, 1)).any()


def test_regression_quantiles_refuse_too_many_samples(dev):
    y = torch.zeros((1025, 4, 1), device=dev)
    with pytest.raises(bnn_hip.BnnHipError):
        ops.mc_predictive(y, "regression", quantiles=[0.5])
    out = ops.mc_predictive(y, "regression")                                        # the moments have no such cap
    torch.cuda.synchronize()
    assert float(out.variance.abs().max()) == 0.0


@pytest.mark.parametrize("lr", [False, True])
def test_regression_equals_the_reference_loop(dev, lr):
    """regression/reg_task.py:76-83 (S calls of net(x, sample=True) collected into [S, N]) through the oracle on the same
    injected epsilon, then np.percentile at 0/25/50/75/100 (utils/plot_utils.py:8-29), the mean and the variance."""
    B, S = 400, 10
    net, sd = build_net(dev, lr, (1, 400, 1), "regression", B=B)
    x, _ = synth.synth_batch("regression", B, 1, 1)
    x = np.asarray(x, np.float32).reshape(B, 1)
    p = O.NetParams.from_state_dict(sd, "regression", 1, lr, O.Prior.from_init([1.0], False))
    outs = np.stack([O.network_forward(p, torch.from_numpy(x), [torch.from_numpy(a) for a in synth.synth_eps(p.eps_shapes(B), s)])[0]
                     .numpy().reshape(B) for s in range(S)])                        # [S, N]
    install_eps(net, B, S, lr)
    got = net.predictive(torch.from_numpy(x).to(dev), S, quantiles=[0, .25, .5, .75, 1], sigma=0.1)
    scale = np.abs(outs).max()
    np.testing.assert_allclose(got.quantiles.cpu().numpy()[..., 0], np.percentile(outs, [0, 25, 50, 75, 100], axis=0),
                               rtol=1e-4, atol=1e-5 * scale)
    np.testing.assert_allclose(got.mean.cpu().numpy()[:, 0], outs.mean(0), rtol=1e-4, atol=1e-5 * scale)
    np.testing.assert_allclose(got.variance.cpu().numpy()[:, 0], outs.astype(np.float64).var(0), rtol=1e-4, atol=1e-6 * scale ** 2)
    np.testing.assert_allclose(got.predictive_variance.cpu().numpy()[:, 0], outs.astype(np.float64).var(0) + 0.01, rtol=1e-4)
    assert got.probs is None and got.preds is None


@pytest.mark.parametrize("lr", [False, True])
def test_classification_equals_predict_mc_and_the_float64_entropies(dev, lr):
    B, S = 128, 6
    net, sd = build_net(dev, lr, (784, 1200, 10), "classification")
    x = torch.from_numpy(synth.synth_batch("classification", B, 784, 10)[0]).to(dev)
    install_eps(net, B, S, lr)
    preds_mc, probs_mc = net.predict_mc(x, S)
    install_eps(net, B, S, lr)
    logits = net.forward_mc(x, S)
    install_eps(net, B, S, lr)
    got = net.predictive(x, S)
    torch.cuda.synchronize()
    np.testing.assert_allclose(got.probs.cpu().numpy(), probs_mc.cpu().numpy(), rtol=0, atol=1e-6)
    probs, pe, ee, mi = np_classification(logits.cpu().numpy()[None])
    check_preds(got.preds.cpu().numpy(), probs[0])
    check_preds(preds_mc.cpu().numpy(), probs[0])
    np.testing.assert_allclose(got.predictive_entropy.cpu().numpy(), pe[0], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(got.expected_entropy.cpu().numpy(), ee[0], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(got.mutual_information.cpu().numpy(), mi[0], rtol=0, atol=2e-5)
    assert got.mean is None and got.quantiles is None


def _close(a, b, tol, what):
    for f, x, y in zip(a._fields, a, b):
        if x is None:
            assert y is None, f
            continue
        if f == "preds":
            continue                                         # near-ties may flip between the two launch chains
        # (bf16 math: the entropies are sums over the classes of p log p -- a few times the probabilities' rounding)
        t = tol * (4 if f.endswith(("entropy", "information")) else 1)
        err = float((x.double() - y.double()).abs().max())
        assert err <= t * max(1.0, float(y.double().abs().max())), (what, f, err)


@pytest.mark.parametrize("lr", [False, True])
def test_predictive_graph_replays_eager_predictive_with_fresh_epsilon(dev, lr):
    """net.predictive_graph (hipGraph and recorded launches): every replay equals the eager net.predictive at the same Philox
    sample indices; consecutive replays draw fresh epsilon, and a new input copied into `.x` changes the answer."""
    B, S, seed, c = 128, 10, 20261, 700
    net, _ = build_net(dev, lr, (784, 1200, 10), "classification")
    xs = [torch.from_numpy(synth.synth_batch("classification", B, 784, 10, seed=50 + m)[0]).to(dev).view(B, 784) for m in range(2)]
    for math, tol in (("f32", 2e-5), ("bf16", 6e-3)):
        bnn_hip.set_math(math)
        for capture in (True, "calls"):
            bnn_hip.manual_seed(seed, counter=c)
            g = net.predictive_graph(xs[0].clone(), S, capture=capture)
            pre = 1 if capture is True else 2               # evaluations construction ran (warm-up, + the recorded pass)
            got = [tuple(t.clone() if t is not None else None for t in g.replay()) for _ in range(2)]
            g.x.copy_(xs[1])
            other = g.replay()
            other = tuple(t.clone() if t is not None else None for t in other)
            torch.cuda.synchronize()
            assert int(g.counter.item()) == c + (pre + 3) * S
            for k, r in enumerate(got):
                bnn_hip.manual_seed(seed, counter=c + (pre + k) * S)
                _close(ops.Predictive(*r), net.predictive(xs[0], S), tol, (math, capture, k))
                assert torch.equal(r[1], r[0].argmax(-1))
            assert float((got[0][0] - got[1][0]).abs().max()) > 1e-4                  # fresh epsilon
            bnn_hip.manual_seed(seed, counter=c + (pre + 2) * S)
            _close(ops.Predictive(*other), net.predictive(xs[1], S), tol, (math, capture, "x"))
            assert float((other[0] - got[1][0]).abs().max()) > 1e-4                   # the new input counts


@pytest.mark.parametrize("lr", [False, True])
def test_regression_graph_with_quantiles_replays_eager(dev, lr):
    B, S, seed, c = 400, 10, 20262, 300
    net, _ = build_net(dev, lr, (1, 400, 1), "regression", B=B)
    x = torch.from_numpy(np.asarray(synth.synth_batch("regression", B, 1, 1)[0], np.float32).reshape(B, 1)).to(dev)
    q = [0.0, 0.25, 0.5, 0.75, 1.0]
    for capture in (True, "calls"):
        bnn_hip.manual_seed(seed, counter=c)
        g = net.predictive_graph(x, S, quantiles=q, sigma=0.1, capture=capture)
        pre = 1 if capture is True else 2
        r = tuple(t.clone() if t is not None else None for t in g.replay())
        torch.cuda.synchronize()
        bnn_hip.manual_seed(seed, counter=c + pre * S)
        _close(ops.Predictive(*r), net.predictive(x, S, quantiles=q, sigma=0.1), 2e-5, capture)
        assert tuple(r[-1].shape) == (5, B, 1)


@pytest.mark.parametrize("mode", ["classification", "regression"])
def test_stacked_replay_equals_single_minibatch_evaluations(dev, mode):
    """A stacked evaluation of G = 4 minibatches: minibatch g draws the sample indices [c + g S, c + (g + 1) S) -- the same
    summaries as four one-minibatch evaluations started there."""
    G, B, S, seed, c = 4, 128, 10, 20263, 100
    dims = (784, 1200, 10) if mode == "classification" else (1, 400, 1)
    net, _ = build_net(dev, False, dims, mode, B=B)
    xs = torch.stack([torch.from_numpy(np.asarray(synth.synth_batch(mode, B, dims[0], dims[2], seed=60 + m)[0], np.float32))
                      .reshape(B, dims[0]) for m in range(G)]).to(dev)
    kw = dict(quantiles=[0.1, 0.5, 0.9]) if mode == "regression" else {}
    bnn_hip.manual_seed(seed, counter=c)
    st = net.predictive(xs, S, stacked=True, **kw)
    torch.cuda.synchronize()
    assert bnn_hip.runtime.state.counter == c + G * S
    for gi in range(G):
        bnn_hip.manual_seed(seed, counter=c + gi * S)
        one = net.predictive(xs[gi], S, **kw)
        part = ops.Predictive(*(None if t is None else (t[:, gi] if f == "quantiles" else t[gi]) for f, t in zip(st._fields, st)))
        _close(part, one, 2e-5, gi)
