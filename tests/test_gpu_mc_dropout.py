"""MC dropout of MLP_Dropout on the device (bnn_dense_fwd / bnn_dropout_mask, MLP_Dropout.mc_forward / predict_mc /
predictive / predictive_graph) against the numpy restatement of the kind-3 dropout map and fp64 torch forwards that
apply the restated masks.
Layer-level accuracy of bnn_dense_fwd, element by element, lives in tests/test_gpu_dense_layer.py."""
import numpy as np
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

import bnn_hip
from bnn_hip import ops
from bnn_hip.runtime import state
from test_mc_dropout_cpu import dropout_mask_np

SEED = 0x5EED0123456789AB


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore():
    yield
    bnn_hip.set_math("bf16")
    bnn_hip.manual_seed(2026)


def _mlp(dev, inp, hidden, out, mode, seed=0):
    import networks
    torch.manual_seed(seed)
    m = networks.MLP_Dropout(dict(input_shape=inp, classes=out, batch_size=128, hidden_units=hidden, mode=mode))
    return m.to(dev)


def _input(dev, mlp, B, seed=1):
    g = torch.Generator().manual_seed(seed)
    if mlp.mode == "classification":
        return torch.rand((B, 1, 28, 28), generator=g).to(dev)
    return torch.randn((B, mlp.input_shape), generator=g).to(dev)


def ref_forward(mlp, x, S, first, seed, bf16=False):
    """fp64 forward of S MC-dropout passes with the restated masks; bf16: operands rounded to bf16 as the kernel
    rounds them (x and W at every layer, the hidden activations stored in bf16)."""
    h = x.reshape(x.shape[0], -1).double()
    if bf16:
        h = h.to(torch.bfloat16).double()
    h = h.unsqueeze(0).expand(S, -1, -1)
    mods = list(mlp.net)
    lins = [i for i, m in enumerate(mods) if isinstance(m, nn.Linear)]
    for l, i in enumerate(lins):
        W, b = mods[i].weight.detach(), mods[i].bias.detach()
        Wd = (W.to(torch.bfloat16) if bf16 else W).double()
        z = h @ Wd.T + b.double()
        if i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU):
            z = torch.relu(z)
        p = mods[i + 2].p if i + 2 < len(mods) and isinstance(mods[i + 2], nn.Dropout) else 0.0
        if p:
            B, N = z.shape[1], z.shape[2]
            m = np.stack([dropout_mask_np(seed, l, first + s, B, N, p) for s in range(S)])
            z = z * torch.from_numpy(m).to(z.device).double()
        if bf16 and l < len(lins) - 1:
            z = z.float().to(torch.bfloat16).double()
        h = z
    return h


def _close(got, ref, tol):
    scale = ref.abs().max().item()
    err = (got.double() - ref).abs().max().item()
    assert err <= tol * max(scale, 1e-30), (err, scale)


@pytest.mark.parametrize("layer,offset,rows,cols,p", [(0, 0, 128, 1200, 0.5), (1, 17, 5, 37, 0.5), (2, 2 ** 31 + 5, 9, 13, 0.1),
                                                       (7, 3, 33, 6, 0.9), (0, 0, 4, 3, 0.0)])
@pytest.mark.parametrize("seed", [0, SEED, 12345])
def test_dropout_mask_equals_the_restatement_bitwise(dev, layer, offset, rows, cols, p, seed):
    S = 3
    got = ops.dropout_mask(seed, layer, offset, S, rows, cols, p, dev).cpu().numpy()
    want = np.stack([dropout_mask_np(seed, layer, offset + s, rows, cols, p) for s in range(S)])
    assert np.array_equal(got, want)


NETS = [("classification", 784, 1200, 10, 128), ("regression", 1, 400, 1, 400), ("regression", 13, 37, 3, 5)]


def _f32_cases():
    out = [(NETS[0], S) for S in (1, 10, 64)]
    return out + [(NETS[1], 10), (NETS[2], 10)]


@pytest.mark.parametrize("net,S", _f32_cases())
def test_f32_mc_forward_equals_the_fp64_restatement(dev, net, S):
    mode, inp, hid, out, B = net
    bnn_hip.set_math("f32")
    mlp = _mlp(dev, inp, hid, out, mode)
    x = _input(dev, mlp, B)
    bnn_hip.manual_seed(SEED, 1000)
    y = mlp.mc_forward(x, S)
    assert y.shape == (S, B, out) and y.dtype == torch.float32
    _close(y, ref_forward(mlp, x, S, 1000, SEED), 1e-5)


@pytest.mark.parametrize("net,S,B", [(NETS[0], 10, 128), (NETS[1], 10, 400), (NETS[2], 10, 5), (NETS[0], 8, 1000)])
def test_bf16_mc_forward_equals_the_rounding_point_restatement(dev, net, S, B):
    mode, inp, hid, out, _ = net
    bnn_hip.set_math("bf16")
    mlp = _mlp(dev, inp, hid, out, mode)
    x = _input(dev, mlp, B)
    bnn_hip.manual_seed(SEED, 77)
    y = mlp.mc_forward(x, S)
    _close(y, ref_forward(mlp, x, S, 77, SEED, bf16=True), 2e-3)


def test_p0_is_the_eval_network_and_has_no_mutual_information(dev):
    bnn_hip.set_math("f32")
    mlp = _mlp(dev, 784, 1200, 10, "classification")
    for m in mlp.net:
        if isinstance(m, nn.Dropout):
            m.p = 0.0
    x = _input(dev, mlp, 128)
    y = mlp.mc_forward(x, 6)
    mlp.eval()
    with torch.no_grad():
        want = mlp(x).double()
    for s in range(6):
        _close(y[s], want, 1e-5)
    assert torch.equal(y[0], y[5])
    pr = mlp.predictive(x, 6)
    assert pr.mutual_information.abs().max().item() <= 1e-6


@pytest.mark.parametrize("math_mode", ["f32", "bf16"])
def test_predictive_is_mc_predictive_over_mc_forward(dev, math_mode):
    bnn_hip.set_math(math_mode)
    mlp = _mlp(dev, 784, 1200, 10, "classification")
    x = _input(dev, mlp, 128)
    bnn_hip.manual_seed(SEED, 40)
    pr = mlp.predictive(x, 10)
    bnn_hip.manual_seed(SEED, 40)
    y = mlp.mc_forward(x, 10)
    want = ops.mc_predictive(y, "classification")
    for f in ("probs", "preds", "predictive_entropy", "expected_entropy", "mutual_information"):
        assert torch.equal(getattr(pr, f), getattr(want, f)[0]), f
    bnn_hip.manual_seed(SEED, 40)
    preds, probs = mlp.predict_mc(x, 10)
    assert torch.allclose(probs, pr.probs, rtol=0, atol=1e-6)        # (bnn_mc_softmax_mean: its own summation order)
    assert torch.equal(preds, torch.argmax(probs, -1))
    # entropies against fp64 from the logits
    z = y.double()
    ps = torch.softmax(z, -1)
    pm = ps.mean(0)
    pe = -(pm * torch.log(pm)).sum(-1)
    ee = -(ps * torch.log_softmax(z, -1)).sum(-1).mean(0)
    assert torch.allclose(pr.probs.double(), pm, atol=1e-6)
    assert torch.allclose(pr.predictive_entropy.double(), pe, atol=1e-5)
    assert torch.allclose(pr.expected_entropy.double(), ee, atol=1e-5)
    assert torch.allclose(pr.mutual_information.double(), torch.clamp(pe - ee, min=0), atol=1e-5)


def test_regression_predictive_quantiles_are_numpy_percentiles(dev):
    bnn_hip.set_math("f32")
    mlp = _mlp(dev, 1, 400, 1, "regression")
    x = _input(dev, mlp, 400)
    q = (0.05, 0.25, 0.5, 0.75, 0.95)
    bnn_hip.manual_seed(SEED, 9)
    pr = mlp.predictive(x, 10, quantiles=q, sigma=0.5)
    bnn_hip.manual_seed(SEED, 9)
    y = mlp.mc_forward(x, 10)
    want = ops.mc_predictive(y, "regression", quantiles=q, sigma=0.5)
    for f in ("mean", "variance", "predictive_variance"):
        assert torch.equal(getattr(pr, f), getattr(want, f)[0]), f
    assert torch.equal(pr.quantiles, want.quantiles[:, 0])
    ref = np.percentile(y.cpu().numpy().astype(np.float64), [100 * v for v in q], axis=0)
    assert np.allclose(pr.quantiles.cpu().numpy(), ref, rtol=1e-6, atol=1e-6)


def test_counter_semantics(dev):
    bnn_hip.set_math("bf16")
    mlp = _mlp(dev, 784, 1200, 10, "classification")
    x = _input(dev, mlp, 128)
    bnn_hip.manual_seed(SEED, 500)
    a = mlp.mc_forward(x, 10)
    b = mlp.mc_forward(x, 10)
    assert state.counter == 520
    assert not torch.equal(a, b)
    bnn_hip.manual_seed(SEED, 510)
    assert torch.equal(mlp.mc_forward(x, 10), b)
    bnn_hip.manual_seed(SEED, 500)
    parts = torch.cat([mlp.mc_forward(x, 4), mlp.mc_forward(x, 6)])
    same = True                                       # the later layers' tiles at 4, 6 and 10 samples
    for lin in (mlp.net[3], mlp.net[6]):
        tiles = {ops.dense_plan(torch.empty((S, 128, lin.in_features), dtype=torch.bfloat16, device=dev), lin.weight, lin.bias,
                                n_samples=S, math_mode=1, relu=True, drop_p=0.0, layer_id=0, seed=0)["batch_rows"]
                 for S in (4, 6, 10)}
        same &= len(tiles) == 1
    if same:
        assert torch.equal(parts, a)
    else:
        _close(parts, a.double(), 2e-3)


@pytest.mark.parametrize("capture", [True, False])
@pytest.mark.parametrize("mode", ["classification", "regression"])
def test_predictive_graph_replays_equal_eager_predictive(dev, capture, mode):
    bnn_hip.set_math("bf16")
    if mode == "classification":
        mlp, kw, B = _mlp(dev, 784, 1200, 10, mode), {}, 128
    else:
        mlp, kw, B = _mlp(dev, 1, 400, 1, mode), dict(quantiles=(0.1, 0.5, 0.9), sigma=0.3), 400
    x = _input(dev, mlp, B)
    bnn_hip.manual_seed(SEED, 3000)
    S = 10
    g = mlp.predictive_graph(x, S, capture=capture, **kw)
    got, counters = [], []
    for _ in range(3):
        counters.append(state.counter)
        got.append([None if t is None else t.clone() for t in g.replay()])
    assert counters[1] == counters[0] + S and counters[2] == counters[1] + S
    for c, out in zip(counters, got):
        bnn_hip.manual_seed(SEED, c)
        want = mlp.predictive(x, S, **kw)
        for f, a, b in zip(want._fields, out, want):
            assert (a is None) == (b is None), f
            if a is not None:
                assert torch.equal(a, b), (f, c)
    first = 0 if mode == "classification" else 5             # probs / mean: fresh masks on every replay
    assert not torch.equal(got[0][first], got[1][first])
    x2 = _input(dev, mlp, B, seed=5)
    g.x.copy_(x2.reshape(g.x.shape))
    c = state.counter
    out = [None if t is None else t.clone() for t in g.replay()]
    bnn_hip.manual_seed(SEED, c)
    want = mlp.predictive(x2, S, **kw)
    for f, a, b in zip(want._fields, out, want):
        if a is not None:
            assert torch.equal(a, b), f


def test_an_sgd_step_is_seen_by_the_next_evaluation(dev):
    bnn_hip.set_math("f32")
    mlp = _mlp(dev, 784, 1200, 10, "classification")
    x = _input(dev, mlp, 128)
    bnn_hip.manual_seed(SEED, 60)
    before = mlp.mc_forward(x, 4)
    opt = torch.optim.SGD(mlp.parameters(), lr=0.5)
    mlp.train()
    loss = nn.functional.cross_entropy(mlp(x), torch.arange(128, device=dev) % 10)
    loss.backward()
    opt.step()
    bnn_hip.manual_seed(SEED, 60)
    after = mlp.mc_forward(x, 4)
    assert not torch.equal(before, after)
    _close(after, ref_forward(mlp, x, 4, 60, SEED), 1e-5)


def test_forward_is_still_torchs_sequential(dev):
    mlp = _mlp(dev, 784, 1200, 10, "classification")
    x = _input(dev, mlp, 16)
    for train in (True, False):
        mlp.train(train)
        torch.manual_seed(3)
        a = mlp(x)
        torch.manual_seed(3)
        b = mlp.net(x.view(-1, 784))
        assert torch.equal(a, b)
    mlp.eval()
    mlp.enable_dropout()
    assert all(m.training for m in mlp.net if isinstance(m, nn.Dropout))
