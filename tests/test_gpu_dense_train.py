"""Training MLP / MLP_Dropout on the device (bnn_dense_fwd -> bnn_dense_loss -> bnn_dense_bwd -> bnn_sgd_step /
bnn_adam_step, bnn_hip.dense_train.GraphedDenseTrainStep) against fp64 restatements on the restated dropout masks,
against itself (graph replays vs eager launches) and against the reference's PyTorch loop.
Layer-level accuracy of bnn_dense_fwd / bnn_dense_bwd, element by element, lives in tests/test_gpu_dense_layer.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

pytestmark = pytest.mark.gpu

import bnn_hip
from bnn_hip import ops
from bnn_hip.optim import FusedAdam, FusedSGD
from bnn_hip.runtime import state
from test_dense_train_cpu import dense_loss_np
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


def _mlp(dev, inp, hidden, out, mode, dropout=True, seed=0):
    import networks
    torch.manual_seed(seed)
    cls = networks.MLP_Dropout if dropout else networks.MLP
    return cls(dict(input_shape=inp, classes=out, batch_size=128, hidden_units=hidden, mode=mode)).to(dev)


def _batch(dev, mlp, B, seed=1):
    g = torch.Generator().manual_seed(seed)
    C = mlp.classes
    if mlp.mode == "classification":
        x = torch.rand((B, 1, 1, mlp.input_shape), generator=g)          # [batch, 1, h, w] as the reference feeds it
        return x.to(dev), torch.randint(0, C, (B,), generator=g).to(dev)
    return torch.randn((B, mlp.input_shape), generator=g).to(dev), torch.randn((B, C), generator=g).to(dev)


def _lins(mlp):
    mods = list(mlp.net)
    out = []
    for i, m in enumerate(mods):
        if isinstance(m, nn.Linear):
            relu = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
            p = mods[i + 2].p if i + 2 < len(mods) and isinstance(mods[i + 2], nn.Dropout) else 0.0
            out.append((m, relu, p))
    return out


def ref_forward(params, lins, x, index, bf16=False):
    """fp64 activations of every layer with the restated masks of global sample index `index` (bf16: x and W rounded)."""
    h = x.reshape(x.shape[0], -1).double()
    acts = []
    for l, ((W, b), (_, relu, p)) in enumerate(zip(params, lins)):
        hin = h.float().to(torch.bfloat16).double() if bf16 else h
        Wd = (W.to(torch.bfloat16) if bf16 else W).double()
        z = hin @ Wd.T + b.double()
        if relu:
            z = torch.relu(z)
        if p:
            m = dropout_mask_np(state.seed, l, index, z.shape[0], z.shape[1], p)
            z = z * torch.from_numpy(m).to(z.device).double()
        acts.append(z)
        h = z
    return acts


def ref_backward(params, lins, x, acts, g_logits, bf16=False):
    """fp64 gradients [(gW, gb)] at the kernel's rounding points from the kernel's own activations `acts` (fp32): gz of a
    hidden layer is the input gradient above it times (act > 0 ? scale : 0); g_x rounds gz and W to bf16 in bf16 math."""
    grads = [None] * len(params)
    gz = g_logits.double()
    for l in range(len(params) - 1, -1, -1):
        hin = (x.reshape(x.shape[0], -1) if l == 0 else acts[l - 1]).double()
        grads[l] = (gz.T @ hin, gz.sum(0))
        if l:
            W = params[l][0]
            gzr = gz.float().to(torch.bfloat16).double() if bf16 else gz
            Wr = (W.to(torch.bfloat16) if bf16 else W).double()
            _, relu, p = lins[l - 1]
            scale = float(ops.dropout_params(p)[1])
            gz = (gzr @ Wr) * torch.where(acts[l - 1] > 0, scale, 0.0).double() if relu else gzr @ Wr
    return grads


def _close(got, ref, tol, what=""):
    ref = ref.double()
    scale = ref.abs().max().item()
    err = (got.double() - ref).abs().max().item()
    assert err <= tol * max(scale, 1e-30), (what, err, scale)


CONFIGS = [  # (input, hidden, classes, mode, dropout, batch, optimiser)
    (784, 1200, 10, "classification", True, 128, "sgd"),     # ClassConfig MLP_Dropout
    (1, 400, 1, "regression", True, 128, "adam"),            # RegConfig MCDropout_Regression
    (119, 100, 1, "regression", False, 5, "adam"),           # the bandit's greedy agent shape, a ragged batch
    (119, 100, 1, "regression", True, 5, "sgd"),
]


def _opt(kind, mlp, lr=None):
    if kind == "sgd":
        return FusedSGD(mlp.parameters(), lr=lr or 1e-4, weight_decay=1e-3, capturable=True)
    return FusedAdam(mlp.parameters(), lr=lr or 1e-3, capturable=True)


@pytest.mark.parametrize("math_mode,tol_fwd", [("f32", 1e-5), ("bf16", 2e-3)])
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}-b{c[5]}-{c[6]}{'-drop' if c[4] else ''}")
def test_one_step_against_the_fp64_restatement(dev, cfg, math_mode, tol_fwd):
    inp, hid, C, mode, dropout, B, kind = cfg
    bnn_hip.set_math(math_mode)
    bnn_hip.manual_seed(SEED, 4242)
    mlp = _mlp(dev, inp, hid, C, mode, dropout)
    opt = _opt(kind, mlp)
    x, y = _batch(dev, mlp, B)
    lins = _lins(mlp)
    params = [(l.weight.detach().clone(), l.bias.detach().clone()) for l, _, _ in lins]
    s = mlp.graphed_train_step(opt, x, y)
    index = state.counter
    loss = s.step(x, y).item()
    acts = [a[0].clone() for a in s.acts]
    bf16 = math_mode == "bf16"
    ref_acts = ref_forward(params, lins, x, index, bf16=bf16)
    for l, (a, r) in enumerate(zip(acts, ref_acts)):
        _close(a, r, tol_fwd, f"activation {l}")
    # loss and logits' gradient from the kernel's logits: fp32 throughout
    z = acts[-1].double().cpu().numpy()
    ref_loss, ref_g = dense_loss_np(z, y.cpu().numpy(), mode)
    assert abs(loss - ref_loss) <= 1e-5 * max(abs(ref_loss), 1.0), (loss, ref_loss)
    _close(s.g_logits, torch.from_numpy(ref_g).to(dev), 1e-5, "g_logits")
    grads = ref_backward(params, lins, x, acts, s.g_logits, bf16=bf16)
    for l, ((gW, gb), (lin, _, _)) in enumerate(zip(grads, lins)):
        # the output layer's gradients are fp32 throughout; below it they carry the bf16 input gradient in bf16 math
        tol = 1e-5 if (not bf16 or l == len(lins) - 1) else 2e-3
        _close(lin.weight.grad, gW, tol, f"gW{l}")
        _close(lin.bias.grad, gb, tol, f"gb{l}")
    # the update, restated from the kernel's own gradients
    for (W0, b0), (lin, _, _) in zip(params, lins):
        for p0, p in ((W0, lin.weight), (b0, lin.bias)):
            g = p.grad.double()
            if kind == "sgd":
                ref = p0.double() - 1e-4 * (g + 1e-3 * p0.double())
            else:
                m, v = 0.1 * g, 0.001 * g * g
                ref = p0.double() - 1e-3 * (m / 0.1) / ((v / 0.001).sqrt() + 1e-8)
            _close(p.detach(), ref, 1e-5, "update")


def _state_of(opt):
    sd = opt.state_dict()
    out = {}
    for k, st in sd["state"].items():
        for n, v in st.items():
            out[(k, n)] = v.detach().clone() if torch.is_tensor(v) else v
    return out


def _run(dev, kind, capture, steps, seed_counter=900):
    bnn_hip.set_math("f32")
    bnn_hip.manual_seed(SEED, seed_counter)
    mlp = _mlp(dev, 119, 100, 10, "classification", True, seed=5)
    opt = _opt(kind, mlp, lr=1e-3)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=5, gamma=0.5)
    xs = [_batch(dev, mlp, 64, seed=10 + i) for i in range(steps)]
    s = mlp.graphed_train_step(opt, *xs[0], capture=capture)
    out = []
    for i in range(steps):
        loss = s.step(*xs[i]).clone()
        sched.step()
        snap = ([p.detach().clone() for p in mlp.parameters()], loss, _state_of(opt), opt.param_groups[0]["lr"])
        out.append(snap)
    return mlp, opt, s, out


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_graph_replays_match_eager_launches_bitwise(dev, kind):
    _, _, _, graphed = _run(dev, kind, True, 10)
    _, _, _, eager = _run(dev, kind, False, 10)
    assert graphed[3][3] != graphed[5][3]                 # StepLR changed the rate midway
    for i, (g, e) in enumerate(zip(graphed, eager)):
        for a, b in zip(g[0], e[0]):
            assert torch.equal(a, b), i
        assert torch.equal(g[1], e[1]), i
        assert g[2].keys() == e[2].keys()
        for k in g[2]:
            assert (torch.equal(g[2][k], e[2][k]) if torch.is_tensor(g[2][k]) else g[2][k] == e[2][k]), (i, k)
    _, _, _, again = _run(dev, kind, True, 10)
    for a, b in zip(graphed[-1][0], again[-1][0]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_building_the_step_leaves_model_and_optimiser_unchanged(dev, kind):
    bnn_hip.set_math("f32")
    mlp = _mlp(dev, 119, 100, 10, "classification", True, seed=5)
    opt = _opt(kind, mlp, lr=1e-3)
    x, y = _batch(dev, mlp, 64)
    # an optimiser with history: one eager step first (so a second, 96-row-like object is built on a trained one)
    first = mlp.graphed_train_step(opt, x, y, capture=False)
    first.step(x, y)
    before_p = [p.detach().clone() for p in mlp.parameters()]
    before_s = _state_of(opt)
    counter = state.counter
    mirror = opt._sample_words["mirror"]
    mlp.graphed_train_step(opt, x[:48], y[:48])
    torch.cuda.synchronize()
    for a, b in zip(before_p, mlp.parameters()):
        assert torch.equal(a, b.detach())
    after_s = _state_of(opt)
    assert before_s.keys() == after_s.keys()
    for k in before_s:
        assert (torch.equal(before_s[k], after_s[k]) if torch.is_tensor(before_s[k]) else before_s[k] == after_s[k]), k
    assert state.counter == counter and opt._sample_words["mirror"] == mirror
    assert int(opt._sample_words["counter"].item()) == mirror


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_a_step_built_after_an_lr_change_trains_at_the_new_rate(dev, kind):
    """The second object's warm-up step is the first launch to see the halved rate: undoing it must not leave the device
    word at the old rate with the new one taken for written.  Against the same launches issued eagerly (no warm-up)."""
    def run(capture):
        bnn_hip.set_math("f32")
        bnn_hip.manual_seed(SEED, 300)
        mlp = _mlp(dev, 8, 16, 4, "classification", False, seed=11)
        opt = _opt(kind, mlp, lr=1e-2)
        x, y = _batch(dev, mlp, 8)
        mlp.graphed_train_step(opt, x, y, capture=capture).step(x, y)
        opt.param_groups[0]["lr"] = 5e-3
        before = [p.detach().clone() for p in mlp.parameters()]
        mlp.graphed_train_step(opt, x[:5], y[:5], capture=capture).step(x[:5], y[:5])
        return before, [p.detach().clone() for p in mlp.parameters()]

    start_g, graphed = run(True)
    start_e, eager = run(False)
    for s, t, a, b in zip(start_g, start_e, graphed, eager):
        assert torch.equal(s, t) and torch.equal(a, b) and not torch.equal(a, s)


def _ref_torch_loop(mlp, opt, x, y, masks):
    """The reference's train_step body on stock torch modules; masks (one per dropout layer) stand in for nn.Dropout."""
    opt.zero_grad()
    h = x.reshape(x.shape[0], -1)
    mi = 0
    for m in mlp.net:
        if isinstance(m, nn.Dropout):
            h = h * masks[mi]
            mi += 1
        else:
            h = m(h)
    loss = F.cross_entropy(h, y, reduction="sum")
    loss.backward()
    opt.step()
    return loss.detach()


@pytest.mark.parametrize("dropout", [False, True])
def test_twenty_steps_match_the_reference_torch_loop(dev, dropout):
    """f32 math: 20 steps of (c) against the reference loop (cross_entropy(sum), torch.optim.SGD) on a copy of the same
    network, with the restated masks multiplied in where the reference has nn.Dropout."""
    bnn_hip.set_math("f32")
    bnn_hip.manual_seed(SEED, 31)
    mlp = _mlp(dev, 784, 256, 10, "classification", dropout, seed=3)
    ref = _mlp(dev, 784, 256, 10, "classification", dropout, seed=3)
    ref.load_state_dict(mlp.state_dict())
    opt = FusedSGD(mlp.parameters(), lr=1e-4, capturable=True)      # ClassConfig's rate
    ropt = torch.optim.SGD(ref.parameters(), lr=1e-4)
    batches = [_batch(dev, mlp, 128, seed=100 + i) for i in range(20)]
    s = mlp.graphed_train_step(opt, *batches[0])
    lins = _lins(mlp)
    for i, (x, y) in enumerate(batches):
        index = state.counter
        masks = [torch.from_numpy(dropout_mask_np(state.seed, l, index, 128, lin.out_features, p)).to(dev)
                 for l, (lin, _, p) in enumerate(lins) if p]
        got = s.step(x, y).item()
        want = _ref_torch_loop(ref, ropt, x, y, masks).item()
        assert abs(got - want) <= 2e-4 * abs(want), (i, got, want)
    # tolerance: the two fp32 products sum in different orders, so a pre-activation within rounding of 0 may open the ReLU
    # in one and not the other -- one row's gradient then differs in full (about lr * |gz x|, under 1e-4 of the weights'
    # scale at this rate); the rest differs at the 1e-6 level
    for a, b in zip(mlp.parameters(), ref.parameters()):
        _close(a.detach(), b.detach(), 2e-4)


def test_counter_semantics(dev):
    bnn_hip.set_math("f32")
    bnn_hip.manual_seed(SEED, 5000)
    mlp = _mlp(dev, 119, 64, 10, "classification", True, seed=7)
    opt = FusedSGD(mlp.parameters(), lr=0.0, capturable=True)      # lr 0: the parameters stay, the masks move
    x128, y128 = _batch(dev, mlp, 128)
    full = mlp.graphed_train_step(opt, x128, y128)
    last = mlp.graphed_train_step(opt, x128[:96], y128[:96])
    assert full.counter is last.counter
    lins = _lins(mlp)
    params = [(l.weight.detach().clone(), l.bias.detach().clone()) for l, _, _ in lins]
    seen = []
    for i in range(6):
        s, xb = (full, x128) if i % 3 != 2 else (last, x128[:96])
        index = state.counter
        seen.append(index)
        s.step(xb, y128[:xb.shape[0]])
        ref = ref_forward(params, lins, xb, index)
        _close(s.acts[0][0], ref[0], 1e-5, f"step {i}")
        _close(s.acts[1][0], ref[1], 1e-5, f"step {i}")
    assert len(set(seen)) == len(seen) and seen == list(range(seen[0], seen[0] + 6))
    m0 = dropout_mask_np(state.seed, 0, seen[0], 128, 64, 0.5)
    m1 = dropout_mask_np(state.seed, 0, seen[1], 128, 64, 0.5)
    assert not np.array_equal(m0, m1)
    sh = opt._sample_words
    assert int(sh["counter"].item()) == sh["mirror"] == (state.counter - sh["base"]) & 0xFFFFFFFF
    assert state.counter == seen[-1] + 1
    # a following MC-dropout evaluation draws past the training's indices
    out = mlp.mc_forward(x128, 2)
    assert state.counter == seen[-1] + 3
    for s_ in range(2):
        ref = ref_forward(params, lins, x128, seen[-1] + 1 + s_)
        _close(out[s_], ref[-1], 1e-5, "mc_forward")
    mlp.predictive(x128, 4)
    assert state.counter == seen[-1] + 7
    # evaluations between steps are skipped by the next step, not reused
    index = state.counter
    full.step(x128, y128)
    _close(full.acts[0][0], ref_forward(params, lins, x128, index)[0], 1e-5, "after evaluation")


def test_out_of_range_label_gives_nan_and_no_fault(dev):
    bnn_hip.set_math("f32")
    for bad in (10, -1, 1 << 40):
        mlp = _mlp(dev, 119, 32, 10, "classification", True)
        opt = FusedSGD(mlp.parameters(), lr=1e-3, capturable=True)
        x, y = _batch(dev, mlp, 16)
        s = mlp.graphed_train_step(opt, x, y)
        assert torch.isfinite(s.step(x, y)).item()
        yb = y.clone()
        yb[3] = bad
        loss = s.step(x, yb)
        torch.cuda.synchronize()
        assert torch.isnan(loss).item()
        assert torch.isnan(s.g_logits[3]).all() and torch.isfinite(s.g_logits[torch.arange(16, device=dev) != 3]).all()


def test_end_to_end_training_learns(dev):
    """Graphed training on bnn_hip.synth inputs with a learnable (teacher) labelling: the loss falls and the MC-dropout
    prediction beats chance clearly."""
    from bnn_hip import synth
    bnn_hip.set_math("bf16")
    bnn_hip.manual_seed(SEED, 0)
    C, inp, N = 4, 64, 512
    x_np, _ = synth.synth_batch("classification", N, inp, C)
    teacher = np.random.RandomState(9).standard_normal((inp, C)).astype(np.float32)
    xf = x_np.reshape(N, -1)
    y_np = np.argmax((xf - xf.mean(0)) @ teacher, axis=1).astype(np.int64)
    x, y = torch.from_numpy(x_np).to(dev), torch.from_numpy(y_np).to(dev)
    mlp = _mlp(dev, inp, 128, C, "classification", True, seed=11)
    opt = FusedAdam(mlp.parameters(), lr=1e-3, capturable=True)
    s = mlp.graphed_train_step(opt, x[:128], y[:128])
    losses = []
    for it in range(400):
        b = (it % 4) * 128
        losses.append(s.step(x[b:b + 128], y[b:b + 128]).item())
    assert np.mean(losses[-20:]) < 0.5 * np.mean(losses[:4]), (losses[:4], losses[-20:])
    acc = (mlp.predictive(x, 10).preds == y).float().mean().item()
    assert acc > 0.6, acc                                  # chance: 0.25
