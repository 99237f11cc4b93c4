"""Training a deep ensemble on the device, every member per launch (bnn_ens_fwd -> bnn_ens_loss -> bnn_ens_bwd ->
bnn_sgd_step / bnn_adam_step over the bank, bnn_hip.ensemble; include/bnn_hip.h F21): each launch bit for bit against the
single-network launch on every member's operands, whole steps against M independent K6 steps, graph replays against eager
launches, one step against torch autograd in fp64, an epoch against the host loop, and the bank's consumers after training.

Shapes: the smallest at which the kernels can still go wrong -- 37-70-65-10 at batch 70 (nothing a multiple of 4 or 64: a
partial second tile, the scalar load paths), 1-40-40-1 at batch 5 (regression), and all widths 64 at batch 64 (exact tiles,
the 16-byte paths; the network class always has three Linears, so the 64-64-64 net is 64-64-64-64); M in {1, 3, 9} (9 is more
than the 8 XCD ranges: the last range is ragged); dropout 0 and 0.5."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

pytestmark = pytest.mark.gpu

import bnn_hip
from bnn_hip import _lib as L
from bnn_hip import ops
from bnn_hip.epoch import DeviceDataset, DeviceLoader, EpochRunner
from bnn_hip.ops import BnnHipError
from bnn_hip.optim import FusedAdam, FusedSGD
from bnn_hip.runtime import state
from test_gpu_dense_train import _close
from test_mc_dropout_cpu import dropout_mask_np

SEED = 0x5EED0123456789AB
SHAPES = {  # name: (widths, mode, batch)
    "c37": ((37, 70, 65, 10), "classification", 70),
    "r1": ((1, 40, 40, 1), "regression", 5),
    "c64": ((64, 64, 64, 64), "classification", 64),
}
MEMBERS = (1, 3, 9)
MATH = {"f32": L.MATH_F32, "bf16": L.MATH_BF16}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore():
    yield
    bnn_hip.set_math("bf16")
    bnn_hip.manual_seed(2026)
    bnn_hip.shard_samples(False)


def _net(dev, shape, dropout, seed=0):
    """An MLP / MLP_Dropout with the layer widths of SHAPES[shape] (the class builds equal hidden widths: the Sequential is
    rebuilt with the wanted ones)."""
    import networks
    widths, mode, _ = SHAPES[shape]
    torch.manual_seed(seed)
    cls = networks.MLP_Dropout if dropout else networks.MLP
    net = cls(dict(input_shape=widths[0], classes=widths[-1], batch_size=128, hidden_units=widths[1], mode=mode))
    mods = []
    for a, b in zip(widths[:-2], widths[1:-1]):
        mods += [nn.Linear(a, b), nn.ReLU()] + ([nn.Dropout(0.5)] if dropout else [])
    net.net = nn.Sequential(*mods, nn.Linear(widths[-2], widths[-1]))
    return net.to(dev)


def _batch(dev, net, B, seed=1, members=None):
    g = torch.Generator().manual_seed(seed)
    lead = () if members is None else (members,)
    if net.mode == "classification":
        x = torch.rand(lead + (B, 1, 1, net.input_shape), generator=g)
        return x.to(dev), torch.randint(0, net.classes, lead + (B,), generator=g).to(dev)
    return torch.randn(lead + (B, net.input_shape), generator=g).to(dev), torch.randn(lead + (B, net.classes), generator=g).to(dev)


def _randn(dev, shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dev)


def _ens(dev, shape, dropout, M, seed0=100):
    net = _net(dev, shape, dropout)
    return net, net.ensemble(M, seeds=range(seed0, seed0 + M))


def _padding_mask(bank):
    m = torch.ones(bank.stride, dtype=torch.bool, device=bank.device)
    for o, n in zip(bank.offsets, bank.numels):
        m[o:o + n] = False
    return m


def _opt(kind, params, lr=None):
    if kind == "sgd":
        return FusedSGD(params, lr=lr or 1e-2, weight_decay=1e-3, capturable=True)
    return FusedAdam(params, lr=lr or 1e-3, capturable=True)


# ------------------------------------------------------------------------------------------------ 1. the forward
@pytest.mark.parametrize("math_mode", ["f32", "bf16"])
@pytest.mark.parametrize("dropout", [False, True], ids=["nodrop", "drop"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_ens_fwd_is_dense_fwd_per_member_bitwise(dev, shape, dropout, math_mode):
    _, _, B = SHAPES[shape]
    for M in MEMBERS:
        net, ens = _ens(dev, shape, dropout, M)
        bank = ens.bank
        ctr = torch.tensor([5], dtype=torch.int32, device=dev)
        for l, d in enumerate(bank.layers):
            K, N = d.linear.in_features, d.linear.out_features
            xs = {"shared": _randn(dev, (B, K), 10 + l), "own": _randn(dev, (M, B, K), 20 + l)}
            for kind, x in xs.items():
                got = ops.ens_fwd(x, bank.buffer, bank._w_off[l], bank._b_off[l], out_features=N, members=M, relu=d.relu,
                                  drop_p=d.p, layer_id=d.layer_id, seed=SEED, sample_offset=1000, sample_counter=ctr,
                                  math_mode=MATH[math_mode])
                assert got.shape == (M, B, N) and got.dtype == torch.float32 and int(ctr.item()) == 5
                for j in range(M):
                    W, b = bank.views(j)[2 * l], bank.views(j)[2 * l + 1]
                    want = ops.dense_fwd(x if kind == "shared" else x[j], W.contiguous(), b.contiguous(), n_samples=1,
                                         math_mode=MATH[math_mode], relu=d.relu, drop_p=d.p, layer_id=d.layer_id, seed=SEED,
                                         sample_offset=1000 + 5 + j, y_dtype=torch.float32)[0]
                    assert torch.equal(got[j], want), (M, l, kind, j)
                if d.p:                                                    # the members draw different masks
                    assert M == 1 or not torch.equal(got[0] == 0, got[M - 1] == 0)
        # the incrementing launch (the output layer: no dropout) advances the counter by M and draws nothing
        l, d = len(bank.layers) - 1, bank.layers[-1]
        x = _randn(dev, (M, B, d.linear.in_features), 30)
        a = ops.ens_fwd(x, bank.buffer, bank._w_off[l], bank._b_off[l], out_features=d.linear.out_features, members=M,
                        layer_id=d.layer_id, seed=SEED, sample_counter=ctr, sample_counter_inc=M, math_mode=MATH[math_mode])
        assert int(ctr.item()) == 5 + M
        b = ops.ens_fwd(x, bank.buffer, bank._w_off[l], bank._b_off[l], out_features=d.linear.out_features, members=M,
                        layer_id=d.layer_id, seed=SEED, math_mode=MATH[math_mode])
        assert torch.equal(a, b)
        with pytest.raises(BnnHipError):                                   # K5's rule: a launch that increments drops nothing
            ops.ens_fwd(x, bank.buffer, bank._w_off[l], bank._b_off[l], out_features=d.linear.out_features, members=M,
                        drop_p=0.5, sample_counter=ctr, sample_counter_inc=M)


# ------------------------------------------------------------------------------------------------ 2. the loss
@pytest.mark.parametrize("mode,B,C", [("classification", 70, 10), ("classification", 300, 3), ("regression", 5, 1),
                                      ("regression", 70, 7)])
def test_ens_loss_is_dense_loss_per_member_bitwise(dev, mode, B, C):
    for M in MEMBERS:
        z = _randn(dev, (M, B, C), 3) * 3
        g = torch.Generator().manual_seed(4)
        if mode == "classification":
            shared, own = torch.randint(0, C, (B,), generator=g).to(dev), torch.randint(0, C, (M, B), generator=g).to(dev)
        else:
            shared, own = torch.randn((B, C), generator=g).to(dev), torch.randn((M, B, C), generator=g).to(dev)
        for kind, tg in (("shared", shared), ("own", own)):
            loss, gl = ops.ens_loss(z, tg, mode, grad_scale=0.5)
            assert loss.shape == (M,) and gl.shape == (M, B, C)
            for j in range(M):
                wl, wg = ops.dense_loss(z[j], tg if kind == "shared" else tg[j], mode, grad_scale=0.5)
                assert torch.equal(loss[j], wl) and torch.equal(gl[j], wg), (M, kind, j)


def test_a_bad_label_poisons_exactly_one_member(dev):
    M, B, C = 3, 70, 10
    z = _randn(dev, (M, B, C), 3)
    y = torch.randint(0, C, (M, B), generator=torch.Generator().manual_seed(4)).to(dev)
    good_loss, good_g = ops.ens_loss(z, y, "classification")
    for bad in (C, -1, 1 << 40):
        yb = y.clone()
        yb[1, 3] = bad
        loss, g = ops.ens_loss(z, yb, "classification")
        torch.cuda.synchronize()
        assert torch.isnan(loss[1]) and torch.isnan(g[1, 3]).all()
        rows = torch.arange(B, device=dev) != 3
        assert torch.equal(g[1, rows], good_g[1, rows])
        for j in (0, 2):
            assert torch.equal(loss[j], good_loss[j]) and torch.equal(g[j], good_g[j])


# ------------------------------------------------------------------------------------------------ 3. the backward
@pytest.mark.parametrize("math_mode", ["f32", "bf16"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_ens_bwd_is_dense_bwd_per_member_bitwise(dev, shape, math_mode):
    _, _, B = SHAPES[shape]
    for M in MEMBERS:
        net, ens = _ens(dev, shape, False, M)
        bank = ens.bank
        pad = _padding_mask(bank)
        for l, d in enumerate(bank.layers):
            K, N = d.linear.in_features, d.linear.out_features
            gy, ysave = _randn(dev, (M, B, N), 40 + l), _randn(dev, (M, B, N), 50 + l)
            xs = {"own": _randn(dev, (M, B, K), 60 + l), "shared": _randn(dev, (B, K), 70 + l)}
            # (x, g_x, gx_mask, bias, saved output): the step's two forms, then each option off / on
            cases = [("own", True, True, True, False), ("shared", False, False, True, False), ("own", True, False, False, True),
                     ("own", False, False, False, False)]
            for kind, want_gx, mask, bias, use_y in cases:
                x = xs[kind]
                bucket = torch.full((M, bank.stride), 7.0, device=dev)
                gx = torch.full((M, B, K), 7.0, device=dev) if want_gx else None
                ops.ens_bwd(x, gy, bank.buffer, bank._w_off[l], bucket, bank._b_off[l] if bias else None, g_x=gx,
                            y=ysave if use_y else None, y_scale=2.0, gx_mask=mask, gx_scale=2.0, math_mode=MATH[math_mode])
                wo, bo = bank._w_off[l], bank._b_off[l]
                for j in range(M):
                    W = bank.views(j)[2 * l].contiguous()
                    rw, rb = torch.empty((N, K), device=dev), torch.empty((N,), device=dev)
                    rx = torch.empty((B, K), device=dev) if want_gx else None
                    ops.dense_bwd(x if kind == "shared" else x[j], gy[j], W, g_w=rw, g_b=rb if bias else None, g_x=rx,
                                  y=ysave[j] if use_y else None, y_scale=2.0, gx_mask=mask, gx_scale=2.0,
                                  math_mode=MATH[math_mode])
                    case = (M, l, kind, want_gx, mask, bias, use_y, j)
                    assert torch.equal(bucket[j, wo:wo + N * K].view(N, K), rw), case
                    if bias:
                        assert torch.equal(bucket[j, bo:bo + N], rb), case
                    if want_gx:
                        assert torch.equal(gx[j], rx), case
                # everything else of the bucket is untouched: the padding, the other layers, the bias without one
                written = torch.zeros(bank.stride, dtype=torch.bool, device=dev)
                written[wo:wo + N * K] = True
                if bias:
                    written[bo:bo + N] = True
                assert (bucket[:, ~written] == 7.0).all() and (bucket[:, pad] == 7.0).all()


# ------------------------------------------------------------------------------------------------ 4. whole steps
def _train_ens(dev, shape, dropout, M, kind, steps, capture=True, per_member=False, counter=700, math_mode="f32"):
    _, _, B = SHAPES[shape]
    bnn_hip.set_math(math_mode)
    bnn_hip.manual_seed(SEED, counter)
    net, ens = _ens(dev, shape, dropout, M)
    start = ens.bank.buffer.clone()
    opt = _opt(kind, ens.parameters())
    batches = [_batch(dev, net, B, seed=10 + t, members=M if per_member else None) for t in range(steps)]
    step = ens.graphed_train_step(opt, *batches[0], capture=capture)
    snaps = []
    for t in range(steps):
        loss = step.step(*batches[t]).clone()
        st = {k: v.clone() for k, v in opt.state[ens._param].items() if torch.is_tensor(v)}
        snaps.append((ens.bank.buffer.clone(), loss, st))
    return net, ens, opt, step, batches, start, snaps


@pytest.mark.parametrize("kind", ["sgd", "adam"])
@pytest.mark.parametrize("dropout", [False, True], ids=["nodrop", "drop"])
@pytest.mark.parametrize("shape,M,per_member", [("c37", 1, False), ("c37", 3, False), ("c37", 9, False), ("c37", 3, True),
                                                ("r1", 3, False), ("r1", 3, True), ("c64", 9, False)])
def test_three_steps_match_independent_k6_steps_bitwise(dev, shape, M, per_member, dropout, kind):
    """Member j of step t against a GraphedDenseTrainStep on a copy of the member, its sample counter at base + M t + j: the
    bank, the losses and Adam's moments bit for bit; M = 1 is a plain K6 step.  The buffer's padding stays exactly 0."""
    steps, base = 3, 700
    net, ens, opt, step, batches, start, snaps = _train_ens(dev, shape, dropout, M, kind, steps, per_member=per_member, counter=base)
    bank = ens.bank
    assert step.launches == 8 and state.counter == base + M * steps
    assert int(step.counter.item()) == M * steps
    pad = _padding_mask(bank)
    for buf, _, st in snaps:
        assert (buf[:, pad] == 0).all()
        for v in st.values():
            assert (v.view(M, -1)[:, pad] == 0).all()
    assert not torch.equal(snaps[-1][0], start)
    for j in range(M):
        ref = copy.deepcopy(net)
        for v, p in zip([start[j, o:o + n].view(s) for o, n, s in zip(bank.offsets, bank.numels, bank.shapes)], bank._params_of(ref)):
            p.data.copy_(v)
        ropt = _opt(kind, ref.parameters())
        state.counter = base + j
        rstep = ref.graphed_train_step(ropt, *[b[j] if per_member else b for b in batches[0]])
        for t in range(steps):
            state.counter = base + M * t + j
            x, y = [b[j] if per_member else b for b in batches[t]]
            loss = rstep.step(x, y)
            buf, losses, st = snaps[t]
            assert torch.equal(loss, losses[j]), (j, t)
            for p, o, n in zip(bank._params_of(ref), bank.offsets, bank.numels):
                assert torch.equal(p.detach().reshape(-1), buf[j, o:o + n]), (j, t)
                if kind == "adam":
                    for key in ("exp_avg", "exp_avg_sq"):
                        assert torch.equal(ropt.state[p][key].reshape(-1), st[key].view(M, -1)[j, o:o + n]), (j, t, key)
    if kind == "adam":
        assert opt.device_step() == steps


# ------------------------------------------------------------------------------------------------ 5. graph vs eager
@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_graph_replays_match_eager_launches_bitwise(dev, kind):
    g = _train_ens(dev, "c37", True, 3, kind, 4, capture=True)
    e = _train_ens(dev, "c37", True, 3, kind, 4, capture=False)
    assert g[3].graph is not None and e[3].graph is None
    for t, ((gb, gl, gs), (eb, el, es)) in enumerate(zip(g[6], e[6])):
        assert torch.equal(gb, eb) and torch.equal(gl, el), t
        assert gs.keys() == es.keys() and all(torch.equal(gs[k], es[k]) for k in gs), t


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_building_the_step_leaves_bank_optimiser_and_counter_unchanged(dev, kind):
    bnn_hip.set_math("f32")
    bnn_hip.manual_seed(SEED, 40)
    net, ens = _ens(dev, "c37", True, 3)
    opt = _opt(kind, ens.parameters())
    x, y = _batch(dev, net, 70)
    first = ens.graphed_train_step(opt, x, y, capture=False)             # an optimiser with history
    first.step(x, y)
    buf = ens.bank.buffer.clone()
    ptr = ens.bank.buffer.data_ptr()
    st = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt.state[ens._param].items()}
    dev_words = [w.clone() if torch.is_tensor(w) else w for w in opt._dev[0]]
    counter, mirror = state.counter, opt._sample_words["mirror"]
    second = ens.graphed_train_step(opt, x[:48], y[:48])
    torch.cuda.synchronize()
    assert second.counter is first.counter
    assert torch.equal(ens.bank.buffer, buf) and ens.bank.buffer.data_ptr() == ptr and ens.bank.count() == 3
    after = opt.state[ens._param]
    assert after.keys() == st.keys()
    for k, v in st.items():
        assert torch.equal(after[k], v) if torch.is_tensor(v) else after[k] == v, k
    for a, b in zip(opt._dev[0], dev_words):
        assert torch.equal(a, b) if torch.is_tensor(b) else a == b
    assert state.counter == counter == 40 + 3 and opt._sample_words["mirror"] == mirror
    assert int(opt._sample_words["counter"].item()) == mirror


# ------------------------------------------------------------------------------------------------ 6. against fp64 autograd
@pytest.mark.parametrize("shape,kind", [("c37", "sgd"), ("r1", "adam"), ("c64", "adam")])
def test_one_f32_step_against_torch_autograd_in_fp64(dev, shape, kind):
    """Per member: activations, loss, logits gradient, parameter gradients and the update against torch autograd in fp64 on
    the restated dropout masks, with tests/test_gpu_dense_train.py's f32 tolerances for the same quantities (1e-5 of the
    reference's largest magnitude; the loss 1e-5 of max(|loss|, 1); the update restated from the kernel's own gradients)."""
    widths, mode, B = SHAPES[shape]
    M, base = 3, 4242
    bnn_hip.set_math("f32")
    bnn_hip.manual_seed(SEED, base)
    net, ens = _ens(dev, shape, True, M)
    bank = ens.bank
    lr = 1e-4 if kind == "sgd" else 1e-3
    opt = _opt(kind, ens.parameters(), lr=lr)
    x, y = _batch(dev, net, B)
    start = bank.buffer.clone()
    step = ens.graphed_train_step(opt, x, y)
    losses = step.step(x, y)
    for j in range(M):
        params = [start[j, o:o + n].view(s).double().requires_grad_() for o, n, s in zip(bank.offsets, bank.numels, bank.shapes)]
        h = x.reshape(B, -1).double()
        acts = []
        for l, d in enumerate(bank.layers):
            h = h @ params[2 * l].T + params[2 * l + 1]
            if d.relu:
                h = torch.relu(h)
            if d.p:
                h = h * torch.from_numpy(dropout_mask_np(state.seed, l, base + j, B, h.shape[1], d.p)).to(dev).double()
            acts.append(h)
        acts[-1].retain_grad()
        loss = F.cross_entropy(acts[-1], y, reduction="sum") if mode == "classification" else F.mse_loss(acts[-1], y.double(), reduction="sum")
        loss.backward()
        for l, a in enumerate(acts):
            _close(step.acts[l][j], a.detach(), 1e-5, f"member {j} activation {l}")
        assert abs(losses[j].item() - loss.item()) <= 1e-5 * max(abs(loss.item()), 1.0), (j, losses[j].item(), loss.item())
        _close(step.g_logits[j], acts[-1].grad, 1e-5, f"member {j} g_logits")
        for t, (p, o, n) in enumerate(zip(params, bank.offsets, bank.numels)):
            g = step.bucket[j, o:o + n]
            _close(g, p.grad.reshape(-1), 1e-5, f"member {j} gradient {t}")
            p0, gd = p.detach().reshape(-1), g.double()
            if kind == "sgd":
                ref = p0 - lr * (gd + 1e-3 * p0)
            else:
                m, v = 0.1 * gd, 0.001 * gd * gd
                ref = p0 - lr * (m / 0.1) / ((v / 0.001).sqrt() + 1e-8)
            _close(bank.buffer[j, o:o + n], ref, 1e-5, f"member {j} update {t}")


# ------------------------------------------------------------------------------------------------ 7. an epoch
def test_an_epoch_is_the_host_loop_bitwise(dev):
    widths, mode, B = SHAPES["c37"]
    M, nb = 3, 4
    g = torch.Generator().manual_seed(8)
    data_x = torch.rand((nb * B, 1, 1, widths[0]), generator=g)
    data_y = torch.randint(0, widths[-1], (nb * B,), generator=g)

    def build():
        bnn_hip.set_math("f32")
        bnn_hip.manual_seed(SEED, 90)
        net, ens = _ens(dev, "c37", True, M)
        opt = _opt("adam", ens.parameters())
        loader = DeviceLoader(DeviceDataset(data_x, data_y, device=dev), B, shuffle=True, seed=77)
        return ens, ens.graphed_train_step(opt, *loader.example()), loader

    ens_a, step_a, loader_a = build()
    hist = EpochRunner(step_a, loader_a).run_epoch()
    assert hist.shape == (nb, M)
    counter_a = state.counter
    ens_b, step_b, loader_b = build()
    host = torch.stack([step_b.step(x, y).clone() for x, y in loader_b])
    assert torch.equal(hist, host) and torch.equal(ens_a.bank.buffer, ens_b.bank.buffer)
    assert state.counter == counter_a == 90 + M * nb
    assert not torch.equal(hist[0], hist[-1])
    x5, y5 = _batch(dev, ens_a.mlp, B, members=M)
    with pytest.raises(BnnHipError, match="shared minibatch"):
        EpochRunner(ens_a.graphed_train_step(_opt("sgd", ens_a.parameters()), x5, y5, capture=False), loader_a)


# ------------------------------------------------------------------------------------------------ 8. the bank's consumers
@pytest.mark.parametrize("math_mode", ["f32", "bf16"])
def test_the_trained_bank_feeds_its_consumers_in_place(dev, math_mode):
    widths, mode, B = SHAPES["c37"]
    M = 3
    bnn_hip.set_math(math_mode)
    bnn_hip.manual_seed(SEED, 10)
    net, ens = _ens(dev, "c37", True, M)
    x, y = _batch(dev, net, B)
    xe, ye = _batch(dev, net, 33, seed=2)
    graph = ens.bank.predictive_graph(xe)                                 # captured before training
    before = graph.replay().probs.clone()
    opt = _opt("adam", ens.parameters(), lr=1e-2)
    step = ens.graphed_train_step(opt, x, y)
    for _ in range(5):
        step.step(x, y)
    logits = ens.bank.forward(xe)
    assert logits.shape == (M, 33, widths[-1])
    hidden = torch.float32 if math_mode == "f32" else torch.bfloat16
    lin_of = lambda n: [m for m in n.net if isinstance(m, nn.Linear)]
    for j in range(M):
        member = ens.member(j)                                           # a copy: the bank's values, not its storage
        assert member is not net
        for l, lin in enumerate(lin_of(member)):
            W, bias = ens.bank.views(j)[2 * l], ens.bank.views(j)[2 * l + 1]
            assert torch.equal(lin.weight.detach(), W) and torch.equal(lin.bias.detach(), bias)
            assert lin.weight.data_ptr() != W.data_ptr()
        hj = xe.reshape(33, -1)
        for l, d in enumerate(ens.bank.layers):
            last = l == len(ens.bank.layers) - 1
            W, b = ens.bank.views(j)[2 * l].contiguous(), ens.bank.views(j)[2 * l + 1].contiguous()
            hj = ops.dense_fwd(hj, W, b, n_samples=1, math_mode=MATH[math_mode], relu=d.relu, drop_p=0.0, layer_id=l, seed=SEED,
                               y_dtype=torch.float32 if last else hidden)[0]
        assert torch.equal(logits[j], hj), j
    pred = ens.bank.predictive(xe)
    assert pred.probs.shape == (33, widths[-1]) and torch.allclose(pred.probs.sum(1), torch.ones(33, device=dev), atol=1e-5)
    sc = ens.bank.score(xe, ye).read()
    assert np.isfinite(sc.lpd)
    after = graph.replay().probs
    assert torch.equal(after, pred.probs) and not torch.equal(after, before)     # the old graph sees the trained weights
    # state_dict / load_state_dict work in place
    sd = ens.state_dict()
    ptr = ens.bank.buffer.data_ptr()
    step.step(x, y)
    assert not torch.equal(ens.bank.buffer, sd["buffer"])
    ens.load_state_dict(sd)
    assert torch.equal(ens.bank.buffer, sd["buffer"]) and ens.bank.buffer.data_ptr() == ptr == ens.parameters()[0].data_ptr()


def test_seeded_members_are_reset_parameters_under_their_seeds(dev):
    from bnn_hip.ensemble import seeded_copy
    net = _net(dev, "c37", True)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    a, b, c = net.ensemble(3, seeds=[5, 6, 7]), net.ensemble(3, seeds=[5, 6, 7]), net.ensemble(2, seeds=[7, 5])
    assert a.bank.count() == 3 and a.bank.capacity == 3
    assert torch.equal(a.bank.buffer, b.bank.buffer)
    assert torch.equal(a.bank.buffer[0], c.bank.buffer[1]) and torch.equal(a.bank.buffer[2], c.bank.buffer[0])
    assert not torch.equal(a.bank.buffer[0], a.bank.buffer[1]) and not torch.equal(a.bank.buffer[1], a.bank.buffer[2])
    for k, v in net.state_dict().items():
        assert torch.equal(v, before[k])
    for j, s in enumerate([5, 6, 7]):
        ref = copy.deepcopy(net)
        with torch.random.fork_rng():
            torch.manual_seed(s)
            for m in ref.net:
                if isinstance(m, nn.Linear):
                    m.reset_parameters()
        for v, p in zip(a.bank.views(j), a.bank._params_of(ref)):
            assert torch.equal(v, p.detach())
        for v, p in zip(a.bank.views(j), a.bank._params_of(seeded_copy(net, s))):
            assert torch.equal(v, p.detach())
    assert (a.bank.buffer[:, _padding_mask(a.bank)] == 0).all()
    p = a.parameters()
    assert len(p) == 1 and isinstance(p[0], nn.Parameter) and p[0].data_ptr() == a.bank.buffer.data_ptr()
    assert p[0].numel() == 3 * a.bank.stride


# ------------------------------------------------------------------------------------------------ 9. it learns
def test_a_short_run_lowers_every_members_loss_and_members_stay_different(dev):
    from bnn_hip import synth
    bnn_hip.set_math("bf16")
    bnn_hip.manual_seed(SEED, 0)
    widths, mode, _ = SHAPES["c64"]
    M, N, B, C = 3, 256, 64, 4
    x_np, _ = synth.synth_batch("classification", N, widths[0], C)
    teacher = np.random.RandomState(9).standard_normal((widths[0], C)).astype(np.float32)
    xf = x_np.reshape(N, -1)
    y_np = np.argmax((xf - xf.mean(0)) @ teacher, axis=1).astype(np.int64)
    x, y = torch.from_numpy(x_np).to(dev), torch.from_numpy(y_np).to(dev)
    net, ens = _ens(dev, "c64", True, M)
    opt = FusedAdam(ens.parameters(), lr=1e-3, capturable=True)
    step = ens.graphed_train_step(opt, x[:B], y[:B])
    losses = []
    for it in range(300):
        b = (it % 4) * B
        losses.append(step.step(x[b:b + B], y[b:b + B]).clone())
    losses = torch.stack(losses).cpu().numpy()
    first, last = losses[:4].mean(0), losses[-20:].mean(0)
    assert losses.shape == (300, M) and (last < 0.7 * first).all(), (first, last)
    for i in range(M):
        for j in range(i + 1, M):
            assert not torch.equal(ens.bank.buffer[i], ens.bank.buffer[j])
    assert not np.array_equal(losses[-1, 0], losses[-1, 1])
    acc = (ens.bank.predictive(x).preds == y).float().mean().item()
    assert acc > 0.5, acc                                  # chance: 0.25


# ------------------------------------------------------------------------------------------------ 10. refusals
def test_every_refusal_has_its_sentence(dev):
    from bnn_hip.sgmcmc import FusedSGMCMC
    bnn_hip.set_math("f32")
    net, ens = _ens(dev, "c37", True, 2)
    x, y = _batch(dev, net, 70)
    good = lambda: FusedSGD(ens.parameters(), lr=1e-2, capturable=True)
    with pytest.raises(BnnHipError, match="FusedSGMCMC is not supported"):
        ens.graphed_train_step(FusedSGMCMC(ens.parameters(), 1e-3, dataset_size=100, batch_size=10), x, y)
    with pytest.raises(BnnHipError, match="FusedSGD or FusedAdam"):
        ens.graphed_train_step(torch.optim.SGD(ens.parameters(), lr=1e-2), x, y)
    with pytest.raises(BnnHipError, match="capturable"):
        ens.graphed_train_step(FusedSGD(ens.parameters(), lr=1e-2), x, y)
    with pytest.raises(BnnHipError, match="capturable"):
        ens.graphed_train_step(FusedAdam(ens.parameters(), lr=1e-2), x, y)
    with pytest.raises(BnnHipError, match="built on ens.parameters"):
        ens.graphed_train_step(FusedSGD(net.parameters(), lr=1e-2, capturable=True), x, y)
    other = net.ensemble(2, seeds=[1, 2])
    with pytest.raises(BnnHipError, match="built on ens.parameters"):
        ens.graphed_train_step(FusedSGD(other.parameters(), lr=1e-2, capturable=True), x, y)
    two = FusedSGD([dict(params=ens.parameters()), dict(params=other.parameters())], lr=1e-2, capturable=True)
    with pytest.raises(BnnHipError, match="one parameter group"):
        ens.graphed_train_step(two, x, y)
    bnn_hip.shard_samples(True)
    with pytest.raises(BnnHipError, match="sharding is not supported"):
        ens.graphed_train_step(good(), x, y)
    bnn_hip.shard_samples(False)
    with pytest.raises(BnnHipError, match="ROCm device only"):
        ens.graphed_train_step(good(), x.cpu(), y.cpu())
    with pytest.raises(BnnHipError, match="must be one of"):
        ens.graphed_train_step(good(), x, y, loss="hinge")
    with pytest.raises(BnnHipError, match="int64 labels"):
        ens.graphed_train_step(good(), x, y.float())
    # a Dropout without a ReLU before it
    bare = _net(dev, "c37", True)
    bare.net = nn.Sequential(nn.Linear(37, 70), nn.Dropout(0.5), nn.Linear(70, 65), nn.ReLU(), nn.Linear(65, 10)).to(dev)
    be = bare.ensemble(2, seeds=[1, 2])
    with pytest.raises(BnnHipError, match="a Dropout needs a ReLU before it"):
        be.graphed_train_step(FusedSGD(be.parameters(), lr=1e-2, capturable=True), x, y)
    # members missing: the step refuses to build until the bank is full
    empty = net.ensemble(3)
    eopt = FusedSGD(empty.parameters(), lr=1e-2, capturable=True)
    empty.bank.push(net)
    with pytest.raises(BnnHipError, match="holds 1 of 3 members"):
        empty.graphed_train_step(eopt, x, y)
    empty.bank.push(ens.member(0))
    empty.bank.push(ens.member(1))
    s = empty.graphed_train_step(eopt, x, y, capture=False)
    assert torch.isfinite(s.step(x, y)).all()
    with pytest.raises(BnnHipError, match="example's shape"):
        s.step(x[:5], y[:5])
    with pytest.raises(BnnHipError, match="seeds"):
        net.ensemble(3, seeds=[1, 2])
    with pytest.raises(BnnHipError, match="members must be >= 1"):
        net.ensemble(0)
