"""The device epoch loader on an MI355X (bnn_epoch_permutation / bnn_epoch_stage, bnn_hip.epoch, bnn_hip.tasks): the two
kernels against the CPU restatement (tests/epoch_ref.py), whole epochs through EpochRunner against the existing path (a host
loop of step.step over the same minibatches), no host synchronisation in run_epoch, evaluate against the per-minibatch
loop, and the task wrappers against the runner."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bnn_hip
import epoch_ref as R
from bnn_hip import epoch, ops
from bnn_hip.optim import FusedAdam, FusedSGD
from bnn_hip.runtime import state

SEED = 0x5EED0123456789AB
SIZES = (1, 5, 128, 8192, 8193, 60000)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore():
    yield
    bnn_hip.set_math("bf16")
    bnn_hip.manual_seed(2026)


# ---------------------------------------------------------------------------------------------------- 1. the permutation
@pytest.mark.parametrize("N", SIZES)
def test_permutation_equals_the_restatement(dev, N):
    words = torch.zeros(4, dtype=torch.int32, device=dev)
    order = torch.full((N,), -1, dtype=torch.int32, device=dev)
    a = ops.epoch_perm_args(n_rows=N, seed=SEED, epoch=words[1:2], order=order)
    ops.epoch_permutation(a)
    assert np.array_equal(order.cpu().numpy(), R.permutation(SEED, 0, N))
    words[1:2].fill_(7)                                   # the epoch is read from the device word: same block, next launch
    ops.epoch_permutation(a)
    got = order.cpu().numpy()
    assert np.array_equal(got, R.permutation(SEED, 7, N))
    assert N < 5 or not np.array_equal(got, R.permutation(SEED, 0, N))


# ---------------------------------------------------------------------------------------------------- 2. the staging
def _dataset(N, d, u8, labels, k=2, seed=3):
    rs = np.random.RandomState(seed)
    x = rs.randint(0, 256, (N, d)).astype(np.uint8) if u8 else (rs.standard_normal((N, d)) * 3).astype(np.float32)
    y = rs.randint(0, 10, N).astype(np.int64) if labels else rs.standard_normal((N, k)).astype(np.float32)
    return x, y


@pytest.mark.parametrize("order_kind", ["given", "drawn", "none"])
@pytest.mark.parametrize("labels", [True, False])
@pytest.mark.parametrize("d", [1, 119, 784])
@pytest.mark.parametrize("u8", [False, True])
def test_stage_equals_the_restatement(dev, u8, d, labels, order_kind):
    N, B = 333, 32
    M = N // B
    x, y = _dataset(N, d, u8, labels)
    ld = epoch.DeviceLoader(epoch.DeviceDataset(x, y, device=dev), B, shuffle=order_kind != "none", seed=SEED + d)
    if order_kind == "given":
        want = np.random.RandomState(5).permutation(N).astype(np.int32)
        got_order = ld.begin_epoch(torch.from_numpy(want))
    else:
        want = R.permutation(SEED + d, 0, N) if order_kind == "drawn" else None
        got_order = ld.begin_epoch()
    assert (got_order is None) == (want is None)
    if want is not None:
        assert np.array_equal(got_order.cpu().numpy(), want)
    k = 0 if labels else y.shape[1]
    xo = torch.zeros((B, d), dtype=torch.float32, device=dev)
    x16 = torch.zeros((B, d), dtype=torch.bfloat16, device=dev)
    yo = torch.zeros((B,) if labels else (B, k), dtype=torch.int64 if labels else torch.float32, device=dev)
    beta = torch.full((1,), -1.0, dtype=torch.float32, device=dev)
    table = torch.from_numpy(epoch.beta_table(M)).to(dev)
    a = ld.stage_args(xo, yo, want is not None, x_bf16_out=x16, beta_table=table, beta=beta)
    cast_ref = torch.zeros_like(x16)
    for j in range(M):
        assert int(ld.batch_index.item()) == j and int(ld.epoch.item()) == 0
        ops.epoch_stage(a)
        rx, r16, ry, rb = R.stage(x, y, j, B, want, M)
        assert np.array_equal(xo.cpu().numpy().view(np.uint32), rx.view(np.uint32)), j
        assert np.array_equal(x16.view(torch.int16).cpu().numpy().view(np.uint16), r16), j
        assert np.array_equal(yo.cpu().numpy(), ry), j
        assert beta.cpu().numpy()[0] == rb
        # the bf16 copy is what bnn_stage_inputs_cast makes of the same rows
        if (B * d * 4) % 16 == 0:
            ops.stage_inputs(xo.clone(), torch.empty_like(xo), cast0=cast_ref)
            assert torch.equal(cast_ref.view(torch.int16), x16.view(torch.int16))
        else:
            assert torch.equal(xo.to(torch.bfloat16).view(torch.int16), x16.view(torch.int16))
    ld.end_epoch()
    assert int(ld.batch_index.item()) == 0 and int(ld.epoch.item()) == 1          # wrapped after M launches
    assert int(ld._state()[2].item()) == 0                                          # the ticket is left at 0


def test_loader_iteration_yields_the_reference_minibatches(dev):
    N, B = 300, 64
    rs = np.random.RandomState(1)
    x = rs.randint(0, 256, (N, 1, 28, 28)).astype(np.uint8)
    y = rs.randint(0, 10, N).astype(np.int64)
    ld = epoch.DeviceLoader(epoch.DeviceDataset(x, y, device=dev), B, seed=9)
    for e in range(2):
        order = R.permutation(9, e, N)
        got = list(ld)
        assert len(got) == len(ld) == N // B
        for j, (xb, yb) in enumerate(got):
            idx = order[j * B:(j + 1) * B]
            assert tuple(xb.shape) == (B, 1, 28, 28) and xb.dtype == torch.float32
            assert np.array_equal(xb.cpu().numpy(), x[idx].astype(np.float32) / np.float32(255.0))
            assert np.array_equal(yb.cpu().numpy(), y[idx])
    it = iter(ld)                                         # a pass abandoned half-way is rewound by the next one
    next(it)
    del it
    assert len(list(ld)) == len(ld) and int(ld.batch_index.item()) == 0


# ---------------------------------------------------------------------------------------------------- 3. epoch parity
def _bnn(dev, dims, mode, lr, seed):
    import networks
    torch.manual_seed(seed)
    mp = dict(input_shape=dims[0], classes=dims[2], batch_size=8, hidden_units=dims[1], mode=mode, mu_init=[-0.2, 0.2],
              rho_init=[-5, -4], prior_init=[1.0], mixture_prior=False, local_reparam=lr)
    return networks.BayesianNetwork(mp).to(dev).train()


def _mlp(dev, dims, mode, dropout, seed):
    import networks
    torch.manual_seed(seed)
    cls = networks.MLP_Dropout if dropout else networks.MLP
    return cls(dict(input_shape=dims[0], classes=dims[2], batch_size=8, hidden_units=dims[1], mode=mode)).to(dev).train()


def _data(dims, mode, N, seed=4):
    rs = np.random.RandomState(seed)
    if mode == "classification":
        side = int(round(dims[0] ** 0.5))
        shape = (N, 1, side, side) if side * side == dims[0] else (N, 1, 1, dims[0])
        return rs.uniform(0, 1, shape).astype(np.float32), rs.randint(0, dims[2], N).astype(np.int64)
    x = rs.uniform(-1, 1, (N, dims[0])).astype(np.float32)
    return x, (np.sin(3 * x[:, :1]) + 0.1 * rs.standard_normal((N, dims[2]))).astype(np.float32)


CASES = {   # name -> (kind, dims, mode, math, batch, minibatches, MC samples)
    "bbb-bf16": ("bbb", (16, 24, 3), "classification", "bf16", 8, 5, 2),
    "bbb-f32": ("bbb", (16, 24, 3), "classification", "f32", 8, 5, 2),
    "lr-bf16": ("lr", (16, 24, 3), "classification", "bf16", 8, 5, 2),
    "lr-f32": ("lr", (1, 24, 1), "regression", "f32", 16, 4, 3),
    "bbb-bf16-reg": ("bbb", (1, 24, 1), "regression", "bf16", 16, 4, 3),
    "mlp-sgd": ("mlp", (16, 24, 3), "classification", "bf16", 8, 5, 1),
    "dropout-adam": ("dropout", (1, 24, 1), "regression", "f32", 16, 4, 1),
    "classconfig-lr-bf16": ("lr", (784, 1200, 10), "classification", "bf16", 128, 4, 2),
    "classconfig-bbb-bf16": ("bbb", (784, 1200, 10), "classification", "bf16", 128, 4, 2),
}


def _run(dev, case, runner, orders, X, Y):
    """Two epochs from one fixed start (network seed, Philox seed and counter), a StepLR change between them: through
    EpochRunner (`runner`) or as the host loop of step.step over the same minibatches.  Returns everything compared."""
    kind, dims, mode, math_mode, B, M, S = case
    bnn_hip.set_math(math_mode)
    bnn_hip.manual_seed(SEED, counter=1000)
    if kind in ("bbb", "lr"):
        net = _bnn(dev, dims, mode, kind == "lr", 21)
        opt = FusedAdam(net.parameters(), lr=1e-3, capturable=True)
    else:
        net = _mlp(dev, dims, mode, kind == "dropout", 21)
        opt = (FusedAdam(net.parameters(), lr=1e-3, capturable=True) if kind == "dropout"
               else FusedSGD(net.parameters(), lr=1e-3, weight_decay=1e-3, capturable=True))
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    ld = epoch.DeviceLoader(epoch.DeviceDataset(X, Y, device=dev), B, seed=77)
    ex, ey = ld.example()
    if kind in ("bbb", "lr"):
        from bnn_hip.train import GraphedTrainStep
        step = GraphedTrainStep(net, opt, ex, ey, S, sigma=0.1 if mode == "regression" else 1.0)
    else:
        step = net.graphed_train_step(opt, ex, ey)
    hists = []
    Xd, Yd = torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev)
    run = epoch.EpochRunner(step, ld) if runner else None
    for e in range(2):
        if runner:
            hists.append(run.run_epoch(orders[e]).clone())
        else:
            rows = []
            for j in range(M):
                idx = orders[e][j * B:(j + 1) * B].to(dev)
                if kind in ("bbb", "lr"):
                    out = step.step(Xd[idx], Yd[idx], 2 ** (M - (j + 1)) / (2 ** M - 1))
                    rows.append(torch.cat([o.reshape(1) for o in out]))
                else:
                    rows.append(step.step(Xd[idx], Yd[idx]).reshape(1).clone())
            hists.append(torch.stack(rows))
        sched.step()
    torch.cuda.synchronize()
    res = {f"param/{n}": p.detach().clone() for n, p in net.named_parameters()}
    for i, p in enumerate(net.parameters()):
        for key in ("exp_avg", "exp_avg_sq"):
            if key in opt.state.get(p, {}):
                res[f"{key}/{i}"] = opt.state[p][key].clone()
    res["history/0"], res["history/1"] = hists
    res["lr_word"] = (opt._dev[0][0] if kind == "mlp" else opt._dev[0][1]).clone()      # FusedSGD: [lr, ...]; FusedAdam: [step, lr, ...]
    res["counter"] = step.counter.clone().float()
    return res, state.counter


@pytest.mark.parametrize("name", sorted(CASES))
def test_epoch_runner_equals_the_host_loop(dev, name):
    """EpochRunner.run_epoch(order) against the existing path -- step.step(x[idx_j], y[idx_j], beta_j) over the same
    minibatches -- on identical networks, optimisers and Philox indices: parameters, Adam moments, the [M, k] loss history
    of both epochs, the learning-rate word after the StepLR change and the MC-sample counter.  The staging is a copy and a
    cast, so the expectation is BIT EQUALITY.  The host loop is first run twice from the same start: wherever those two
    runs are bit-equal the runner must be bit-equal too; where they are not (a path that accumulates with atomics) the
    bound is 4 x their measured difference, never anything taken from the runner's output.  Measured on an MI355X: the two
    host-loop runs were bit-equal in every case listed here, so every comparison below is exact."""
    case = CASES[name]
    kind, dims, mode, math_mode, B, M, S = case
    N = B * M + 3                                                       # drop_last drops three rows
    X, Y = _data(dims, mode, N)
    g = torch.Generator().manual_seed(13)
    orders = [torch.randperm(N, generator=g) for _ in range(2)]
    ref1, c1 = _run(dev, case, False, orders, X, Y)
    ref2, c2 = _run(dev, case, False, orders, X, Y)
    got, cg = _run(dev, case, True, orders, X, Y)
    assert c1 == c2 == cg == 1000 + 2 * M * S                           # the host's sample counter moved as step() moves it
    worst = 0.0
    for key, a in ref1.items():
        spread = float((a.double() - ref2[key].double()).abs().max())
        diff = float((a.double() - got[key].double()).abs().max())
        worst = max(worst, spread)
        print(f"{name} {key}: host loop twice {spread:.3e}, runner vs host loop {diff:.3e}")
        assert torch.isfinite(a.double()).all(), key
        if spread == 0.0:
            assert torch.equal(a, got[key]), (key, diff)
        else:
            assert diff <= 4.0 * spread, (key, diff, spread)
    print(f"{name}: largest difference between the two host-loop runs {worst:.3e}")


# ---------------------------------------------------------------------------------------------------- 4. no host traffic
@pytest.mark.parametrize("kind", ["lr", "dropout"])
def test_run_epoch_does_not_synchronise(dev, kind):
    """Method: torch.cuda.set_sync_debug_mode("error") -- honoured on ROCm builds of torch (the bandit tests rely on it):
    any synchronising call inside the block (.item(), .cpu(), a stream synchronise through torch) raises."""
    case = (kind, (16, 24, 3), "classification", "bf16", 8, 6, 2)
    X, Y = _data(case[1], case[2], 50)
    bnn_hip.manual_seed(SEED, counter=10)
    ld = epoch.DeviceLoader(epoch.DeviceDataset((X * 255).astype(np.uint8), Y, device=dev), 8, seed=3)
    ex, ey = ld.example()
    if kind == "lr":
        from bnn_hip.train import GraphedTrainStep
        net = _bnn(dev, case[1], case[2], True, 2)
        step = GraphedTrainStep(net, FusedAdam(net.parameters(), lr=1e-3, capturable=True), ex, ey, 2)
    else:
        net = _mlp(dev, case[1], case[2], True, 2)
        step = net.graphed_train_step(FusedAdam(net.parameters(), lr=1e-3, capturable=True), ex, ey)
    run = epoch.EpochRunner(step, ld)
    run.run_epoch()                                       # warm-up: allocations, first launches
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        hist = run.run_epoch()
        hist2 = run.run_epoch()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert tuple(hist.shape) == (6, 3 if kind == "lr" else 1)
    assert torch.isfinite(hist).all() and torch.isfinite(hist2).all() and int(ld.epoch.item()) == 3


# ---------------------------------------------------------------------------------------------------- 5. evaluate
@pytest.mark.parametrize("kind", ["bbb", "lr", "dropout", "mlp"])
def test_evaluate_equals_the_per_minibatch_loop(dev, kind):
    """The correct count of epoch.evaluate against the reference's loop (class_task.py:89-103) over the same minibatches,
    the seeds aligned: both start at the same Philox counter, and minibatch g of a stacked evaluation draws the indices
    the g-th call of the loop draws."""
    dims, B, S, N = (64, 48, 10), 32, 4, 32 * 7 + 5
    X, _ = _data(dims, "classification", N)
    bnn_hip.set_math("f32")
    net = (_bnn(dev, dims, "classification", kind == "lr", 6) if kind in ("bbb", "lr")
           else _mlp(dev, dims, "classification", kind == "dropout", 6)).eval()
    with torch.no_grad():                                 # labels the network gets partly right
        ref_pred = torch.argmax(net(torch.from_numpy(X).to(dev)) if kind in ("mlp", "dropout") else
                                net.predict_mc(torch.from_numpy(X).to(dev), 8)[1], dim=1).cpu().numpy()
    Y = np.where(np.arange(N) % 3 == 0, (ref_pred + 1) % 10, ref_pred).astype(np.int64)
    ld = epoch.DeviceLoader(epoch.DeviceDataset((X * 255).astype(np.uint8), Y, device=dev), B, shuffle=False)
    samples = 0 if kind == "mlp" else S
    bnn_hip.manual_seed(SEED, counter=300)
    got = epoch.evaluate(net, ld, samples, chunk=3)
    end = state.counter
    bnn_hip.manual_seed(SEED, counter=300)
    want = 0
    with torch.no_grad():
        for x, y in ld:
            preds = torch.argmax(net(x), dim=1) if kind == "mlp" else net.predict_mc(x, S)[0]
            want += int((preds == y).sum().item())
    assert got == want and 0 < got < len(ld) * B
    assert end == state.counter == 300 + (0 if kind == "mlp" else len(ld) * S)


# ---------------------------------------------------------------------------------------------------- 6. the wrappers
def test_wrapper_epochs_equal_the_runner_and_the_scheduler_reaches_the_device(dev, tmp_path):
    from bnn_hip import tasks
    from bnn_hip.train import GraphedTrainStep
    N, B = 100, 16
    X, Y = _data((16, 24, 3), "classification", N)
    params = dict(lr=1e-3, hidden_units=24, mode="classification", batch_size=B, num_batches=N // B, train_samples=2,
                  test_samples=3, x_shape=16, classes=3, mu_init=[-0.2, 0.2], rho_init=[-5, -4], prior_init=[1.0],
                  mixture_prior=False, local_reparam=False, dropout=False, save_dir=str(tmp_path / "m"), epochs=2)
    bnn_hip.manual_seed(SEED, counter=50)
    torch.manual_seed(31)
    t = tasks.BNN_Classification("bnn", params)
    t.scheduler = torch.optim.lr_scheduler.StepLR(t.optimiser, step_size=1, gamma=0.5)
    ld = epoch.DeviceLoader(epoch.DeviceDataset(X, Y, device=dev), B, seed=5)
    for _ in range(2):
        t.train_step(ld)
        t.scheduler.step()
    assert len(t.loss_info) == 4 and tuple(t.loss_info[0].shape) == (1,) and tuple(t.loss_history.shape) == (N // B, 4)
    assert float(t.optimiser._dev[0][1].item()) == np.float32(5e-4)      # the second epoch ran at the halved rate
    t.evaluate(epoch.DeviceLoader(epoch.DeviceDataset(X, Y, device=dev), B, shuffle=False))
    assert 0.0 <= t.acc <= 1.0
    hist_t = t.loss_history.clone()

    bnn_hip.manual_seed(SEED, counter=50)
    torch.manual_seed(31)
    import networks
    net = networks.BayesianNetwork(dict(input_shape=16, classes=3, batch_size=B, hidden_units=24, mode="classification",
                                        mu_init=[-0.2, 0.2], rho_init=[-5, -4], prior_init=[1.0], mixture_prior=False,
                                        local_reparam=False)).to(dev).train()
    opt = FusedAdam(net.parameters(), lr=1e-3, capturable=True)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    ld2 = epoch.DeviceLoader(epoch.DeviceDataset(X, Y, device=dev), B, seed=5)
    run = epoch.EpochRunner(GraphedTrainStep(net, opt, *ld2.example(), 2), ld2)
    for _ in range(2):
        hist = run.run_epoch()
        sched.step()
    assert torch.equal(hist, hist_t)
    for (n, a), (_, b) in zip(t.net.named_parameters(), net.named_parameters()):
        assert torch.equal(a, b), n
