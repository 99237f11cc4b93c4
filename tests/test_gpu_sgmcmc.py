"""SG-MCMC and the weight bank on an MI355X (bnn_sgmcmc_noise / bnn_sgmcmc_step / bnn_bank_fwd, bnn_hip.sgmcmc; include/bnn_hip.h
F19) against the numpy restatement (tests/sgmcmc_ref.py): the noise stream, the update rule bit for bit, the step word, the table
and the ring, the stationary law of the two chains of tests/test_sgmcmc_cpu.py run through the kernel, the bank forward bit for
bit against bnn_dense_fwd and against fp64 bounds, and a tiny network sampled end to end (graph replays, eager launches and the
epoch runner give the same bits)."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bnn_hip
import optim_ref as O
import sgmcmc_ref as R
from bnn_hip import _lib as L
from bnn_hip import ops, sgmcmc
from bnn_hip.ops import BnnHipError

SEED = 0x5EED0123456789AB
NUMELS = (1, 37, 70 * 37, 1201, 2 * 4096 + 5)        # the issue's four, and one that spans three chunks of the kernel


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore():
    yield
    bnn_hip.set_math("bf16")
    bnn_hip.manual_seed(2026)


def _words(dev, step=0, collected=0):
    return sgmcmc._word(step, dev), sgmcmc._word(collected, dev), torch.zeros(16, dtype=torch.int32, device=dev)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _same(got, want):
    return np.array_equal(_bits(got).reshape(-1), np.asarray(want, dtype=np.float32).view(np.uint32).reshape(-1))


def _tensors(dev, numels, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    host = [(rng.standard_normal(n) * scale).astype(np.float32) for n in numels]
    return host, [torch.from_numpy(h).to(dev) for h in host]


# ---------------------------------------------------------------------------------------------- 1. the noise stream
@pytest.mark.parametrize("numel", [1, 5, 37, 1201])
@pytest.mark.parametrize("tensor", [0, 15])
@pytest.mark.parametrize("step", [0, 7, 2 ** 32 - 1])
def test_noise_stream_matches_the_restatement(dev, numel, tensor, step):
    got = ops.sgmcmc_noise(SEED, tensor, step, numel, dev).cpu().numpy()
    assert got.shape == (numel,)
    np.testing.assert_allclose(got, R.noise(SEED, tensor, step, numel), atol=5e-5, rtol=0)


def test_noise_of_a_tensor_does_not_depend_on_its_neighbours(dev):
    """p = 0, grad = 0, (a, b, c) = (0, 0, 1): the step leaves p' = eps.  Tensor 0 draws the same values whatever follows it in
    the launch, a tensor's index moves its stream, and both equal bnn_sgmcmc_noise bit for bit."""
    tab = torch.tensor([[0.0, 0.0, 1.0, 0.0]], device=dev)

    def run(numels, k):
        ps = [torch.zeros(n, device=dev) for n in numels]
        step, _, ticket = _words(dev, k)
        ops.sgmcmc_step(ps, [torch.zeros_like(p) for p in ps], table=tab, step=step, ticket=ticket, grad_scale=1.0, tau=0.0,
                        eps_mode=L.EPS_PHILOX, seed=SEED)
        return ps
    a, b = run((37, 1201), 7), run((37, 5, 1201), 7)
    assert torch.equal(a[0], b[0]) and not torch.equal(a[1], b[2])
    assert torch.equal(a[0], ops.sgmcmc_noise(SEED, 0, 7, 37, dev)) and torch.equal(b[2], ops.sgmcmc_noise(SEED, 2, 7, 1201, dev))
    assert torch.equal(a[1], ops.sgmcmc_noise(SEED, 1, 7, 1201, dev)) and torch.equal(b[1], ops.sgmcmc_noise(SEED, 1, 7, 5, dev))


# ---------------------------------------------------------------------------------------------- 2. the update rule
@pytest.mark.parametrize("friction", [None, 0.3])
def test_update_rule_bit_for_bit(dev, friction):
    tab = R.table([0.013, 0.0021], temperature=0.9, friction=friction)
    hp, dp = _tensors(dev, NUMELS, 1, 0.3)
    mom = friction is not None
    dm = [torch.zeros_like(p) for p in dp] if mom else None
    ch = R.Chain(hp, tab, grad_scale=468.75, tau=0.5, momentum=mom)
    step, _, ticket = _words(dev)
    dtab = torch.from_numpy(tab).to(dev)
    zp = [p.clone() for p in dp]
    zm = [torch.zeros_like(p) for p in dp] if mom else None
    zstep, _, zticket = _words(dev)
    for k in range(2):                                           # (the second step starts from a momentum that is not zero)
        hg, dg = _tensors(dev, NUMELS, 10 + k, 0.01)
        he, de = _tensors(dev, NUMELS, 20 + k)
        ch.step(hg, he)
        ops.sgmcmc_step(dp, dg, table=dtab, step=step, ticket=ticket, grad_scale=468.75, tau=0.5, eps_mode=L.EPS_MEMORY,
                        momenta=dm, noise=de)
        for t in range(len(NUMELS)):
            assert _same(dp[t], ch.p[t]), (k, t)
            assert not mom or _same(dm[t], ch.v[t]), (k, t)
    assert sgmcmc._read_word(step) == 2 and int(ticket.abs().sum()) == 0
    # BNN_EPS_ZERO is BNN_EPS_MEMORY fed zeros
    hg, dg = _tensors(dev, NUMELS, 30, 0.01)
    zeros = [torch.zeros_like(p) for p in dp]
    a, b = [p.clone() for p in zp], [p.clone() for p in zp]
    am = [m.clone() for m in zm] if mom else None
    bm = [m.clone() for m in zm] if mom else None
    ops.sgmcmc_step(a, dg, table=dtab, step=zstep, ticket=zticket, grad_scale=468.75, tau=0.5, eps_mode=L.EPS_ZERO, momenta=am)
    s2, _, t2 = _words(dev)
    ops.sgmcmc_step(b, dg, table=dtab, step=s2, ticket=t2, grad_scale=468.75, tau=0.5, eps_mode=L.EPS_MEMORY, momenta=bm, noise=zeros)
    for t in range(len(NUMELS)):
        assert torch.equal(a[t], b[t]) and not torch.equal(a[t], zp[t]) and (not mom or torch.equal(am[t], bm[t]))


@pytest.mark.parametrize("blocks", sorted(O.GRIDS))
@pytest.mark.parametrize("friction", [None, 0.3])
def test_update_rule_bit_for_bit_at_every_grid(dev, friction, blocks):
    """The launch's last block (csrc/bnn_stream.h: 8 ticket groups, then word 0) at grids of 1, 2, 7, 8, 9, 16 and 17 blocks.
    Three launches, flags [0, 1, 1] behind a burn-in of 1 (one launch that does not collect, two that do, capacity 2): after
    every launch the parameters, the momenta and the ring are the restated chain's, the step word has advanced by exactly one,
    the collected word is the chain's and every ticket word is zero."""
    numels = O.GRIDS[blocks]
    assert len(O.chunk_table(numels)) == blocks
    tab = R.table([0.013, 0.0021, 0.0034], temperature=0.9, friction=friction, flags=[0, 1, 1])
    hp, dp = _tensors(dev, numels, 1, 0.3)
    mom = friction is not None
    dm = [torch.zeros_like(p) for p in dp] if mom else None
    hbank = np.full((2, R.layout(numels)[1]), 7.0, dtype=np.float32)
    dbank = torch.from_numpy(hbank.copy()).to(dev)
    ch = R.Chain(hp, tab, grad_scale=468.75, tau=0.5, momentum=mom, burn_in=1, bank=hbank)
    step, collected, ticket = _words(dev)
    dtab = torch.from_numpy(tab).to(dev)
    for k in range(3):
        hg, dg = _tensors(dev, numels, 10 + k, 0.01)
        he, de = _tensors(dev, numels, 20 + k)
        ch.step(hg, he)
        ops.sgmcmc_step(dp, dg, table=dtab, step=step, ticket=ticket, grad_scale=468.75, tau=0.5, eps_mode=L.EPS_MEMORY,
                        momenta=dm, noise=de, burn_in=1, collected=collected, bank=dbank)
        for t in range(len(numels)):
            assert _same(dp[t], ch.p[t]), (k, t)
            assert not mom or _same(dm[t], ch.v[t]), (k, t)
        assert _same(dbank, hbank), k
        assert sgmcmc._read_word(step) == k + 1 == ch.k and sgmcmc._read_word(collected) == k == ch.collected, k
        assert not ticket.any(), k


# ---------------------------------------------------------------------------------------------- 3. PHILOX = MEMORY
@pytest.mark.parametrize("k", [0, 5])
@pytest.mark.parametrize("friction", [None, 0.3])
def test_philox_step_equals_memory_step_on_the_materialised_stream(dev, k, friction):
    tab = torch.from_numpy(R.table([0.02] * 3, friction=friction)).to(dev)
    _, dp = _tensors(dev, NUMELS, 2, 0.3)
    _, dg = _tensors(dev, NUMELS, 3, 0.01)
    mom = friction is not None
    out = []
    for mode in (L.EPS_PHILOX, L.EPS_MEMORY):
        ps = [p.clone() for p in dp]
        ms = [torch.full_like(p, 0.01) for p in dp] if mom else None
        step, _, ticket = _words(dev, k)
        noise = [ops.sgmcmc_noise(SEED, t, k, n, dev) for t, n in enumerate(NUMELS)] if mode == L.EPS_MEMORY else None
        ops.sgmcmc_step(ps, dg, table=tab, step=step, ticket=ticket, grad_scale=468.75, tau=0.5, eps_mode=mode, seed=SEED,
                        momenta=ms, noise=noise)
        assert sgmcmc._read_word(step) == k + 1
        out.append((ps, ms))
    for t in range(len(NUMELS)):
        assert torch.equal(out[0][0][t], out[1][0][t]) and not torch.equal(out[0][0][t], dp[t])
        assert not mom or torch.equal(out[0][1][t], out[1][1][t])


# ---------------------------------------------------------------------------------------------- 4. step word, table, ring
@pytest.mark.parametrize("friction", [None, 0.3])
def test_step_word_table_and_ring(dev, friction):
    """L = 5 distinct step sizes, flags [0, 0, 1, 0, 1], burn_in 3, capacity 2, 12 launches: steps 4, 7 and 9 collect."""
    numels = (37, 70, 4096 + 3)
    tab = R.table([0.011, 0.023, 0.037, 0.041, 0.053], friction=friction, flags=[0, 0, 1, 0, 1])
    offs, stride = R.layout(numels)
    hp, dp = _tensors(dev, numels, 4, 0.3)
    mom = friction is not None
    dm = [torch.zeros_like(p) for p in dp] if mom else None
    hbank = np.full((2, stride), 7.0, dtype=np.float32)
    dbank = torch.from_numpy(hbank.copy()).to(dev)
    ch = R.Chain(hp, tab, grad_scale=2.0, tau=0.5, momentum=mom, burn_in=3, bank=hbank)
    step, collected, ticket = _words(dev)
    dtab = torch.from_numpy(tab).to(dev)
    after = {}
    for k in range(12):
        hg, dg = _tensors(dev, numels, 40 + k, 0.05)
        he, de = _tensors(dev, numels, 60 + k)
        ch.step(hg, he)
        ops.sgmcmc_step(dp, dg, table=dtab, step=step, ticket=ticket, grad_scale=2.0, tau=0.5, eps_mode=L.EPS_MEMORY, momenta=dm,
                        noise=de, burn_in=3, collected=collected, bank=dbank)
        after[k] = [p.clone() for p in dp]
        for t in range(len(numels)):                             # each step used its own row
            assert _same(dp[t], ch.p[t]), (k, t)
    assert sgmcmc._read_word(step) == 12 and sgmcmc._read_word(collected) == 3 == ch.collected
    assert ch.rows_used == [0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 1] and int(ticket.abs().sum()) == 0
    assert _same(dbank, hbank)
    for t, (o, n) in enumerate(zip(offs, numels)):
        assert torch.equal(dbank[0, o:o + n], after[9][t]) and torch.equal(dbank[1, o:o + n], after[7][t])
        assert not torch.equal(after[4][t], after[9][t])
        end = offs[t + 1] if t + 1 < len(offs) else stride
        assert bool((dbank[:, o + n:end] == 7.0).all())          # the padding is untouched
    # without a bank the same chain runs and collects nothing
    step2, col2, ticket2 = _words(dev, 4)
    ops.sgmcmc_step(dp, dg, table=dtab, step=step2, ticket=ticket2, grad_scale=2.0, tau=0.5, eps_mode=L.EPS_ZERO, momenta=dm, burn_in=0)
    assert sgmcmc._read_word(step2) == 5 and sgmcmc._read_word(col2) == 0


# ---------------------------------------------------------------------------------------------- 5. stationary statistics
@pytest.mark.parametrize("name,lr,friction", [("sgld", 0.5, None), ("sghmc", 0.1, 0.3)])
def test_device_chain_samples_the_stationary_law(dev, name, lr, friction):
    """The CPU test's chains through bnn_sgmcmc_step in BNN_EPS_PHILOX: 200 launches on 16 384 elements, the same three bounds
    (a step word that does not advance repeats one noise vector; a scale from the wrong row changes the variance)."""
    n, tau = 16384, 1.0
    tab = sgmcmc.build_table(lr, friction=friction)
    assert np.array_equal(tab, R.table(R.learning_rates(lr, 1), 1.0, friction, [1]))
    p, g = [torch.zeros(n, device=dev)], [torch.zeros(n, device=dev)]
    m = [torch.zeros(n, device=dev)] if friction is not None else None
    step, _, ticket = _words(dev)
    dtab = torch.from_numpy(tab).to(dev)

    def run(k):
        ops.sgmcmc_step(p, g, table=dtab, step=step, ticket=ticket, grad_scale=1.0, tau=tau, eps_mode=L.EPS_PHILOX, seed=SEED,
                        momenta=m)
        return p[0].cpu().numpy()
    var, mean, lag1 = R.chain_statistics(run, n, 200)
    assert sgmcmc._read_word(step) == 200
    ratio, got, want = R.check_statistics(var, mean, lag1, tab[0], tau, n)
    print(f"{name}: var / Sigma_pp = {ratio:.4f}, lag-1 = {got:.4f} against {want:.4f}, mean = {mean:.5f}")


# ---------------------------------------------------------------------------------------------- 6. the bank forward
def _bank_case(dev, B, K, N, M, capacity, first, seed):
    (w_off, b_off), stride = ops.bank_layout([N * K, N])
    rng = np.random.default_rng(seed)
    host = np.full((capacity, stride), np.nan, dtype=np.float32)
    for m in range(first, first + M):
        host[m] = 0.0
        host[m, w_off:w_off + N * K] = rng.standard_normal(N * K) / np.sqrt(K)
        host[m, b_off:b_off + N] = rng.standard_normal(N)
    xs = rng.standard_normal((M, B, K)).astype(np.float32)
    return torch.from_numpy(host).to(dev), w_off, b_off, torch.from_numpy(xs).to(dev)


def _rt_bf16(t):
    return t.to(torch.bfloat16).to(torch.float64)


@pytest.mark.parametrize("shape", [(5, 37, 10), (70, 37, 70), (64, 64, 1), (130, 8, 65)])
@pytest.mark.parametrize("math_mode", ["f32", "bf16"])
def test_bank_forward_equals_dense_fwd_and_the_fp64_product(dev, shape, math_mode):
    B, K, N = shape
    M, capacity, first = 3, 5, 1
    bank, w_off, b_off, xs = _bank_case(dev, B, K, N, M, capacity, first, seed=B + K + N)
    mm = L.MATH_BF16 if math_mode == "bf16" else L.MATH_F32
    variants = [(torch.float32, torch.float32)]
    if math_mode == "bf16":
        variants += [(torch.float32, torch.bfloat16), (torch.bfloat16, torch.float32), (torch.bfloat16, torch.bfloat16)]
    for shared in (True, False):
        for bias in (True, False):
            for relu in (True, False):
                for xdt, ydt in variants:
                    x = (xs[0] if shared else xs).to(xdt).contiguous()
                    y = ops.bank_fwd(x, bank, w_off, b_off if bias else None, out_features=N, members=M, first=first, relu=relu,
                                     math_mode=mm, y_dtype=ydt)
                    assert y.shape == (M, B, N) and y.dtype == ydt
                    what = (shared, bias, relu, xdt, ydt)
                    assert bool(torch.isfinite(y.float()).all()), what     # (the NaN slots outside [first, first + M) are not read)
                    for j in range(M):
                        W = bank[first + j, w_off:w_off + N * K].view(N, K)
                        b = bank[first + j, b_off:b_off + N] if bias else None
                        xj = x if shared else x[j]
                        want = ops.dense_fwd(xj, W, b, n_samples=1, math_mode=mm, relu=relu, drop_p=0.0, layer_id=0, seed=0, y_dtype=ydt)
                        assert torch.equal(y[j], want[0]), (what, j)
                        if ydt != torch.float32:
                            continue
                        # independent of K5: the fp64 product of the operands as the math mode takes them
                        xd = _rt_bf16(xj) if math_mode == "bf16" else xj.double()
                        Wd = _rt_bf16(W) if math_mode == "bf16" else W.double()
                        ref = xd @ Wd.T + (b.double() if bias else 0.0)
                        mag = xd.abs() @ Wd.abs().T + (b.double().abs() if bias else 0.0)
                        if relu:
                            ref = torch.relu(ref)
                        err = (y[j].double() - ref).abs()
                        bound = (K + 2) * 2.0 ** -24 * mag
                        assert bool((err <= bound).all()), (what, j, float((err / bound.clamp_min(1e-300)).max()))
    # first = 0 selects the NaN slot: the result says so
    y0 = ops.bank_fwd(xs[0], bank, w_off, b_off, out_features=N, members=2, first=0, math_mode=mm)
    assert bool(torch.isnan(y0[0]).all()) and torch.equal(y0[1], ops.bank_fwd(xs[0], bank, w_off, b_off, out_features=N, members=1,
                                                                                first=1, math_mode=mm)[0])
    with pytest.raises(BnnHipError):
        ops.bank_fwd(xs[0], bank, w_off, b_off, out_features=N, members=M, first=capacity - M + 1, math_mode=mm)


# ---------------------------------------------------------------------------------------------- 7. end to end, tiny
def _net(dev, mode, seed=0):
    import networks
    torch.manual_seed(seed)
    if mode == "classification":
        mp = dict(input_shape=5, classes=3, batch_size=8, hidden_units=16, mode=mode)
    else:
        mp = dict(input_shape=1, classes=1, batch_size=8, hidden_units=16, mode=mode)
    return networks.MLP(mp).to(dev)


def _data(dev, mode, n=64):
    g = torch.Generator().manual_seed(5)
    if mode == "classification":
        return torch.randn((n, 1, 1, 5), generator=g).to(dev), torch.randint(0, 3, (n,), generator=g).to(dev)
    x = torch.randn((n, 1), generator=g)
    return x.to(dev), (torch.sin(2 * x) + 0.1 * torch.randn((n, 1), generator=g)).to(dev)


def _sampler(net, friction):
    return net.sgmcmc(1e-3, capacity=3, dataset_size=64, batch_size=8, burn_in=2, thin=2, friction=friction, seed=SEED)


def _snapshot(net, opt, bank):
    mom = []                                                     # (a momentum not created yet is a zero momentum)
    if opt.param_groups[0]["friction"] is not None:
        mom = [opt.state[p]["momentum"].clone() if "momentum" in opt.state.get(p, {}) else torch.zeros_like(p)
               for p in net.parameters()]
    return ([p.detach().clone() for p in net.parameters()], mom, bank.buffer.clone(), sgmcmc._read_word(bank.step),
            sgmcmc._read_word(bank.collected))


def _equal(a, b):
    return (all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and len(a[1]) == len(b[1]) and
            all(torch.equal(x, y) for x, y in zip(a[1], b[1])) and torch.equal(a[2], b[2]) and a[3:] == b[3:])


def _member_stack(bank, xf, M):
    """[M, B, out] built member by member with bnn_dense_fwd on the bank's views."""
    from bnn_hip.mcdropout import _math
    mm, hidden = _math()
    outs = []
    for m in range(M):
        v = bank.views(m)
        h = xf
        for i, d in enumerate(bank.layers):
            last = i == len(bank.layers) - 1
            h = ops.dense_fwd(h, v[2 * i], v[2 * i + 1], n_samples=1, math_mode=mm, relu=d.relu, drop_p=0.0, layer_id=i, seed=0,
                              y_dtype=torch.float32 if last else hidden)[0]
        outs.append(h)
    return torch.stack(outs)


@pytest.mark.parametrize("mode", ["classification", "regression"])
@pytest.mark.parametrize("friction", [None, 0.2])
def test_tiny_network_end_to_end(dev, mode, friction):
    from bnn_hip import epoch
    from bnn_hip.dense_train import GraphedDenseTrainStep
    X, Y = _data(dev, mode)
    base = _net(dev, mode)
    runs, steps = {}, {}
    for how in ("graph", "eager", "runner"):
        net = copy.deepcopy(base)
        opt, bank = _sampler(net, friction)
        before = _snapshot(net, opt, bank)
        step = GraphedDenseTrainStep(net, opt, X[:8], Y[:8], capture=how != "eager")
        assert (step.graph is not None) == (how != "eager")
        assert _equal(_snapshot(net, opt, bank), before), how                 # building leaves no trace
        if friction is not None and how != "eager":                           # (the warm-up created the momentum: zero again)
            assert all(float(opt.state[p]["momentum"].abs().max()) == 0.0 for p in net.parameters())
        if how == "runner":
            loader = epoch.DeviceLoader(epoch.DeviceDataset(X, Y), 8, shuffle=False)
            hist = epoch.EpochRunner(step, loader).run_epoch()
            assert hist.shape == (8, 1) and bool(torch.isfinite(hist).all())
        else:
            for j in range(8):
                loss = step.step(X[8 * j:8 * j + 8], Y[8 * j:8 * j + 8])
            assert bool(torch.isfinite(loss))
        runs[how] = (net, opt, bank, _snapshot(net, opt, bank))
        steps[how] = step
    snap = runs["graph"][3]
    assert _equal(snap, runs["eager"][3]) and _equal(snap, runs["runner"][3])
    # steps 3, 5 and 7 collected (burn_in 2, every second step); the weights moved; the last member is the final state
    assert snap[3] == 8 and snap[4] == 3 and len(snap[1]) == (0 if friction is None else 6)
    net, opt, bank, _ = runs["graph"]
    assert bank.count() == 3 and opt.device_step() == 8
    assert all(not torch.equal(p, q) for p, q in zip(snap[0], base.parameters()))
    assert all(torch.equal(v, p) for v, p in zip(bank.views(2), net.parameters()))
    assert not torch.equal(bank.views(0)[0], bank.views(1)[0])

    # summaries: the bank's one-launch-per-layer forward against the stack built member by member
    x, y = X[:8], Y[:8]
    for math_mode in ("f32", "bf16"):
        bnn_hip.set_math(math_mode)
        stack = _member_stack(bank, x.reshape(8, -1), 3)
        assert torch.equal(bank.forward(x), stack)
        want = ops.mc_predictive(stack, mode, sigma=0.7, quantiles=(0.1, 0.9) if mode == "regression" else ())
        kw = dict(quantiles=[0.1, 0.9]) if mode == "regression" else {}
        got = bank.predictive(x, sigma=0.7, **kw)
        graphed = bank.predictive_graph(x, sigma=0.7, **kw)
        rep = graphed.replay()
        assert graphed.graph is not None
        for f, a in zip(want._fields, want):
            if a is None:
                assert getattr(got, f) is None
                continue
            a = a[:, 0] if f == "quantiles" else a[0]
            assert torch.equal(getattr(got, f), a) and torch.equal(getattr(rep, f), a), (math_mode, f)
        s_got, s_want = bank.score(x, y, sigma=0.7), ops.mc_score(stack, y, mode, sigma=0.7)
        assert torch.equal(s_got.record, s_want.record) and s_got.read().n == 8
        if mode == "classification":
            preds, probs = bank.predict_mc(x)
            assert torch.equal(probs, ops.mc_softmax_mean(stack, 1.0 / 3)[0]) and preds.shape == (8,)
        # the data set in one launch and in launches of 24 rows: the same rows scored
        ev = bank.evaluate(epoch.EvalLoader(epoch.DeviceDataset(X, Y), 8), sigma=0.7)
        ev24 = bank.evaluate(epoch.EvalLoader(epoch.DeviceDataset(X, Y), 8), sigma=0.7, rows=24)
        assert ev.read().n == 64 == ev24.read().n

    # a slot round-trips through a network, and the bank through its state dict
    net2 = _net(dev, mode, seed=9)
    assert bank.member(1, into=net2) is net2
    bank2 = net2.weight_bank(3)
    assert bank2.count() == 0 and bank2.push(net2) == 0 and bank2.count() == 1
    assert all(torch.equal(a, b) for a, b in zip(bank2.views(0), bank.views(1)))
    bank2.load_state_dict(bank.state_dict())
    assert torch.equal(bank2.buffer, bank.buffer) and bank2.count() == 3 and sgmcmc._read_word(bank2.step) == 8
    assert bank2.push(net2) == 0 and sgmcmc._read_word(bank2.collected) == 4           # the ring wraps

    # the optimiser's state dict mirrors the step word, and loading keeps the tensors a graph holds
    sd = opt.state_dict()
    assert all(s["step"] == 8 for s in sd["state"].values())
    held = [opt._dev[0][0].data_ptr()] + [opt.state[p]["momentum"].data_ptr() for p in net.parameters() if friction is not None]
    opt.load_state_dict(sd)
    assert held == [opt._dev[0][0].data_ptr()] + [opt.state[p]["momentum"].data_ptr() for p in net.parameters() if friction is not None]
    assert opt.device_step() == 8

    # building a step on a FULL ring: at step word 9 the warm-up step collects over the oldest member -- and is undone
    steps["graph"].step(X[:8], Y[:8])
    full = _snapshot(net, opt, bank)
    assert full[3] == 9 and full[4] == 3 and bank.count() == 3
    GraphedDenseTrainStep(net, opt, X[:8], Y[:8])
    assert _equal(_snapshot(net, opt, bank), full)


def test_refusals(dev):
    from bnn_hip.dense_train import GraphedDenseTrainStep
    X, Y = _data(dev, "classification")
    net = _net(dev, "classification")
    opt = sgmcmc.FusedSGMCMC(net.parameters(), 1e-3, dataset_size=64, batch_size=8, capturable=False)
    with pytest.raises(BnnHipError, match="capturable"):
        GraphedDenseTrainStep(net, opt, X[:8], Y[:8])
    other = _net(dev, "regression").weight_bank(3)
    with pytest.raises(BnnHipError, match="other parameter shapes"):
        sgmcmc.FusedSGMCMC(net.parameters(), 1e-3, dataset_size=64, batch_size=8, bank=other)
    opt2, bank = _sampler(net, None)
    opt2.bank = other                                            # swapped behind the constructor's back
    with pytest.raises(BnnHipError, match="other parameter shapes"):
        GraphedDenseTrainStep(net, opt2, X[:8], Y[:8])
    with pytest.raises(BnnHipError):
        bank.forward(X[:8])                                      # an empty bank predicts nothing
    with pytest.raises(BnnHipError):
        other.member(0, into=net)
