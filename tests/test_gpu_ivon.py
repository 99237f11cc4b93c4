"""IVON on an MI355X (bnn_ivon_draw / bnn_ivon_step, bnn_hip.ivon; include/bnn_hip.h F24) against the numpy restatement
(tests/ivon_ref.py): the draw, the fold and the step bit for bit on given noise across a wrapping draw index, the on-chip stream
against the restated one and the two noise modes and the two destination forms against each other, the bank draws' chunking,
determinism and law, tiny networks trained end to end (graph replays, eager launches, the epoch runner and a host loop that feeds
the restated chain give the same bits), the posterior as a BayesianNetwork and as a bank, the state dict, and the neighbours left
unchanged."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bnn_hip
import ivon_ref as R
import optim_ref as O
from bnn_hip import _lib as L
from bnn_hip import ivon, ops, sgmcmc
from bnn_hip.ops import BnnHipError

SEED = 0x5EED0123456789AB
NUMELS = (1, 5, 37, 1201, 4096, 4100)   # one element, a tail below 4, odd tails, an exact chunk, a chunk plus one float4
SIXTEEN = (3, 64, 65, 130, 7, 1, 4096, 4097, 12, 255, 256, 257, 1023, 2, 5000, 33)
SENTINEL = 7.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore():
    yield
    bnn_hip.set_math("bf16")
    bnn_hip.manual_seed(2026)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _same(got, want):
    return np.array_equal(_bits(got).reshape(-1), np.ascontiguousarray(want, dtype=np.float32).view(np.uint32).reshape(-1))


def _to(dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a).copy()).to(dev)


def _randn(rng, numels, scale=1.0):
    return [(scale * rng.standard_normal(n)).astype(np.float32) for n in numels]


def _rows(rng, ch, rows):
    """[rows, stride] noise: normals where the tensors live, the sentinel in the padding."""
    a = np.full((rows, ch.stride), SENTINEL, dtype=np.float32)
    for sl in ch.sl:
        a[:, sl] = rng.standard_normal((rows, sl.stop - sl.start)).astype(np.float32)
    return a


class _Device:
    """The device side of a restated chain: the chain's arrays copied up, the words beside them."""

    def __init__(self, dev, ch):
        self.p = [_to(dev, t) for t in ch.p]
        self.mean, self.hess, self.gm = _to(dev, ch.mean), _to(dev, ch.hess), _to(dev, ch.gm)
        self.acc_g, self.acc_h = _to(dev, ch.acc_g), _to(dev, ch.acc_h)
        self.step = sgmcmc._word(ch.t, dev)
        self.prod = torch.tensor([ch.prod], dtype=torch.float64, device=dev)
        self.ticket = torch.zeros(16, dtype=torch.int32, device=dev)

    def check(self, ch, where):
        for t in range(len(ch.p)):
            assert _same(self.p[t], ch.p[t]), (where, "param", t)
        for name in ("mean", "hess", "gm") + (("acc_g", "acc_h") if ch.S > 1 else ()):
            assert _same(getattr(self, name), getattr(ch, name)), (where, name)      # (padding included: the sentinel)
        assert sgmcmc._read_word(self.step) == ch.t, where
        assert float(self.prod.item()) == ch.prod, where                               # (the fp64 word's bits)
        assert int(self.ticket.abs().sum()) == 0, where


HYPER = dict(ess=50.0, beta1=0.9, beta2=0.99, weight_decay=1e-3, loss_scale=0.25)


def _chain(numels, S, clip, seed, step0):
    rng = np.random.default_rng(seed)
    prod0 = 0.9 * 0.9 * 0.9
    ch = R.Chain(_randn(rng, numels, 0.5), lr=0.05, samples=S, clip_radius=0.05 if clip else np.inf, step=step0, prod=prod0,
                 pad=SENTINEL, **HYPER)
    for sl in ch.sl:
        ch.hess[sl] = rng.uniform(0.2, 2.0, sl.stop - sl.start).astype(np.float32)
        ch.gm[sl] = (0.1 * rng.standard_normal(sl.stop - sl.start)).astype(np.float32)
    return rng, ch


def _one_step(dev, rng, ch, d, numels, S, clip, lr_word, where, eps_mode=L.EPS_MEMORY, seed=0, noise=None, check=True):
    """Step t of the chain and of the device on the same noise rows and the same gradients."""
    hn = _rows(rng, ch, S) if noise is None else noise
    dn = _to(dev, hn)
    kw = dict(ess=HYPER["ess"], weight_decay=HYPER["weight_decay"], samples=S)
    hg = dg = None
    for s in range(S):
        ops.ivon_draw(d.p, hess=d.hess, mean=d.mean, step=d.step, sample=s, grads=dg, acc_g=d.acc_g if s else None,
                      acc_h=d.acc_h if s else None, eps_mode=eps_mode, seed=seed, noise=dn if eps_mode == L.EPS_MEMORY else None, **kw)
        ch.draw(s, [hn[s, sl] for sl in ch.sl], hg)
        if check:
            d.check(ch, (where, "draw", s))
        hg = _randn(rng, numels, 0.5)
        dg = [_to(dev, g) for g in hg]
    lr_dev = torch.tensor([ch.lr], dtype=torch.float32, device=dev) if lr_word else None
    ops.ivon_step(d.p, dg, lr=123.0 if lr_word else ch.lr, lr_device=lr_dev, beta1=HYPER["beta1"], beta2=HYPER["beta2"],
                  loss_scale=HYPER["loss_scale"], clip_radius=0.05 if clip else float("inf"), mean=d.mean, hess=d.hess,
                  avg_grad=d.gm, acc_g=d.acc_g, acc_h=d.acc_h, step=d.step, beta1_prod=d.prod, ticket=d.ticket, eps_mode=eps_mode,
                  seed=seed, noise=dn if eps_mode == L.EPS_MEMORY else None, **kw)
    ch.step(hg)
    if check:
        d.check(ch, (where, "step"))


# ---------------------------------------------------------------------------------------------- 1. given noise, bit for bit
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("lr_word", [False, True])
def test_draw_and_step_on_given_noise_bit_for_bit(dev, S, clip, lr_word):
    """6 steps from step word 2^32 - 3 over the six tensors: the draw index t * S + s wraps with the word.  After every launch
    the parameters, mean, hess, avg_grad, the accumulators (padding included: the sentinel), the step word, the bits of the fp64
    product and the zeroed ticket are the restated chain's."""
    rng, ch = _chain(NUMELS, S, clip, 1, 2 ** 32 - 3)
    d = _Device(dev, ch)
    hess0 = ch.hess.copy()
    for k in range(6):
        _one_step(dev, rng, ch, d, NUMELS, S, clip, lr_word, k)
    assert ch.t == 3 and not np.array_equal(ch.hess, hess0)
    if clip:                                                # the radius bites for some elements and not for others
        u = np.concatenate([(ch.mean[sl] - ch.p[t].reshape(-1)) / np.float32(ch.lr) for t, sl in enumerate(ch.sl)])
        at = np.isclose(np.abs(u), 0.05, rtol=1e-4)
        assert 0.02 < at.mean() < 0.98, at.mean()


@pytest.mark.parametrize("blocks", sorted(O.GRIDS))
@pytest.mark.parametrize("S", [1, 2])
def test_draw_and_step_on_given_noise_bit_for_bit_at_every_grid(dev, blocks, S):
    """The step launch's last block (csrc/bnn_stream.h: 8 ticket groups, then word 0) at grids of 1, 2, 7, 8, 9, 16 and 17
    blocks.  Three steps: after every launch the state is the restated chain's (_Device.check: the parameters, mean, hess,
    avg_grad, the accumulators, the step word, the bits of the fp64 product, the zeroed ticket), the step word has advanced
    by exactly one per step launch and by nothing in a draw launch, and the product by one factor beta1."""
    numels = O.GRIDS[blocks]
    assert len(O.chunk_table(numels)) == blocks
    rng, ch = _chain(numels, S, True, 6, 5)
    d = _Device(dev, ch)
    for k in range(3):
        prod = ch.prod
        _one_step(dev, rng, ch, d, numels, S, True, False, k)
        assert sgmcmc._read_word(d.step) == 5 + k + 1 == ch.t and float(d.prod.item()) == ch.prod == prod * HYPER["beta1"], k
        assert not d.ticket.any(), k


def test_sixteen_tensors(dev):
    assert len(SIXTEEN) == L.SGMCMC_MAX_TENSORS
    rng, ch = _chain(SIXTEEN, 2, True, 2, 9)
    d = _Device(dev, ch)
    for k in range(2):
        _one_step(dev, rng, ch, d, SIXTEEN, 2, True, False, k)
    assert ch.t == 11


# ---------------------------------------------------------------------------------------------- 2. the on-chip stream
def _device_noise(dev, numels, q, seed, members=1):
    """Draws q .. q + members - 1 of the on-chip stream, materialised through the bank form: mean 0 and ess (h + delta) = 1
    exactly, so sigma = 1 and theta = fma(1, eps, 0) = eps.  [members, stride]; the padding stays 0."""
    stride = R.layout(list(numels))[1]
    bank = torch.zeros((members, stride), dtype=torch.float32, device=dev)
    zeros = [torch.zeros(n, dtype=torch.float32, device=dev) for n in numels]
    ops.ivon_draw(zeros, hess=torch.full((stride,), 0.5, dtype=torch.float32, device=dev), ess=1.0, weight_decay=0.5, bank=bank,
                  members=members, sample_base=q, seed=seed)
    return bank


def test_on_chip_stream_and_the_two_noise_modes(dev):
    """The stream equals the restated one to the 5e-5 every stream test here allows (the device's Box-Muller uses the hardware's
    transcendentals), also across the wrap of the draw index; a Philox-mode chain of two steps at S = 2 equals the memory-mode
    chain on the materialised noise bit for bit; the training-form draw equals the bank-form draw at the same q."""
    S, t0 = 2, 2 ** 31 - 1                                  # q = t0 * 2 + s wraps to 2^32 - 2, 2^32 - 1, 0, 1
    qs = [R.draw_index(t0 + k, S, s) for k in range(2) for s in range(S)]
    assert qs == [2 ** 32 - 2, 2 ** 32 - 1, 0, 1]
    noise = {q: _device_noise(dev, NUMELS, q, SEED)[0].cpu().numpy() for q in qs}
    offs, stride = R.layout(list(NUMELS))
    for q in qs:
        for t, (o, n) in enumerate(zip(offs, NUMELS)):
            np.testing.assert_allclose(noise[q][o:o + n], R.noise(SEED, q, t, n), rtol=0, atol=5e-5)
        assert not noise[q][NUMELS[0]:offs[1]].any()
    two = _device_noise(dev, NUMELS, 2 ** 32 - 1, SEED, members=2).cpu().numpy()            # members of one launch: q, q + 1
    assert np.array_equal(two[0], noise[2 ** 32 - 1]) and np.array_equal(two[1], noise[0])
    assert not np.array_equal(_device_noise(dev, NUMELS, 0, SEED + 1)[0].cpu().numpy(), noise[0])

    _, ch = _chain(NUMELS, S, False, 3, t0)
    a, b = _Device(dev, ch), _Device(dev, ch)
    for k in range(2):
        rows = np.stack([noise[R.draw_index(t0 + k, S, s)] for s in range(S)])
        rng_a, rng_b = np.random.default_rng(40 + k), np.random.default_rng(40 + k)        # (the same gradients)
        ch_b = copy.deepcopy(ch)
        _one_step(dev, rng_a, ch, b, NUMELS, S, False, False, ("memory", k), noise=rows)
        _one_step(dev, rng_b, ch_b, a, NUMELS, S, False, False, ("philox", k), eps_mode=L.EPS_PHILOX, seed=SEED, noise=rows,
                  check=False)
        for x, y in zip(a.p + [a.mean, a.hess, a.gm, a.acc_g, a.acc_h], b.p + [b.mean, b.hess, b.gm, b.acc_g, b.acc_h]):
            assert torch.equal(x, y), k
        assert torch.equal(a.step, b.step) and torch.equal(a.prod, b.prod)

    # the two destination forms at the same q: the training form at (t, s) against the bank form at sample_base = t * S + s
    for s in range(S):
        rng, ch = _chain(NUMELS, S, False, 5, 77)
        d = _Device(dev, ch)
        if s:
            d.mean.copy_(_to(dev, np.concatenate([np.pad(p, (0, -p.size % 64), constant_values=SENTINEL) for p in ch.p])))
        bank = torch.full((3, stride), SENTINEL, dtype=torch.float32, device=dev)
        ops.ivon_draw([p.clone() for p in d.p], hess=d.hess, ess=HYPER["ess"], weight_decay=HYPER["weight_decay"], bank=bank,
                      members=1, first=1, sample_base=R.draw_index(77, S, s), seed=SEED)
        dg = [_to(dev, g) for g in _randn(rng, NUMELS)]
        ops.ivon_draw(d.p, hess=d.hess, mean=d.mean, step=d.step, samples=S, sample=s, grads=dg if s else None,
                      acc_g=d.acc_g if s else None, acc_h=d.acc_h if s else None, ess=HYPER["ess"],
                      weight_decay=HYPER["weight_decay"], seed=SEED)
        for t, (o, n) in enumerate(zip(offs, NUMELS)):
            assert torch.equal(bank[1, o:o + n], d.p[t]), (s, t)
        assert bool((bank[0] == SENTINEL).all()) and bool((bank[2] == SENTINEL).all())      # (other members: not written)
        assert bool((bank[1, NUMELS[0]:offs[1]] == SENTINEL).all())                          # (nor the padding)


# ---------------------------------------------------------------------------------------------- 3. draws into a bank
def _mlp(dev, mode, dropout=False, seed=0):
    import networks
    torch.manual_seed(seed)
    if mode == "classification":
        mp = dict(input_shape=16, classes=3, batch_size=5, hidden_units=8, mode=mode)
    else:
        mp = dict(input_shape=1, classes=1, batch_size=5, hidden_units=40, mode=mode)
    return (networks.MLP_Dropout if dropout else networks.MLP)(mp).to(dev)


def test_sample_bank_chunking_and_determinism(dev):
    net = _mlp(dev, "classification")
    bnn_hip.manual_seed(11, counter=40)
    opt = net.ivon(0.1, 200.0)
    opt.hess.copy_(torch.rand(opt.stride, generator=torch.Generator().manual_seed(3)) + 0.1)
    a = opt.sample_bank(70, sample_offset=100)                                  # 64 + 6
    b = opt.sample_bank(70, sample_offset=100, members_per_launch=1)            # 70 x 1
    assert torch.equal(a.buffer, b.buffer) and a.count() == 70 and a.capacity == 70
    assert torch.equal(opt.sample_bank(5, sample_offset=100, members_per_launch=2).buffer, a.buffer[:5])
    d = opt.sample_bank(5, sample_offset=105)
    assert not torch.equal(a.buffer[:5], d.buffer) and torch.equal(a.buffer[5:10], d.buffer)
    assert bnn_hip.runtime.state.counter == 40                        # (an explicit offset takes nothing from the counter)
    e = opt.sample_bank(3)
    assert bnn_hip.runtime.state.counter == 43 and torch.equal(e.buffer, opt.sample_bank(3, sample_offset=40).buffer)
    # the members scatter around the mean with the posterior's sigma; the mean is the parameters' bits
    for v, p, var in zip(a.views(0), net.parameters(), opt.variance()):
        assert v.shape == p.shape and bool(((v - p.detach()).abs() <= 6 * var.sqrt()).all())
    big = net.weight_bank(8)
    sgmcmc._set_word(big.collected, 7)
    assert opt.sample_bank(5, big, sample_offset=100) is big and sgmcmc._read_word(big.collected) == 7
    assert torch.equal(big.buffer[:5], a.buffer[:5]) and not big.buffer[5:].any()
    bnn_hip.manual_seed(12)
    assert not torch.equal(net.ivon(0.1, 200.0).sample_bank(5, sample_offset=100).buffer, a.buffer[:5])   # (the seed keys the stream)


def test_draw_law(dev):
    """One tensor of 64 elements, 4096 draws (64 launches of 64 members) around a given mean with given sigma.  Per element the
    sample mean lies within 6 standard errors sigma / sqrt(M) of the mean and the sample variance within 6 standard errors
    sigma^2 sqrt(2 / (M - 1)) of sigma^2 (the variance of a Gaussian sample variance); so does the pooled variance of the
    standardised draws, at 6 sqrt(2 / (64 M))."""
    P, M = 64, 4096
    rng = np.random.default_rng(8)
    mean = rng.standard_normal(P).astype(np.float32)
    hess = rng.uniform(0.1, 3.0, P).astype(np.float32)
    bank = torch.zeros((M, P), device=dev)
    for first in range(0, M, L.IVON_MAX_MEMBERS):
        ops.ivon_draw([_to(dev, mean)], hess=_to(dev, hess), ess=30.0, weight_decay=1e-2, bank=bank, members=L.IVON_MAX_MEMBERS,
                      first=first, sample_base=first, seed=SEED)
    X = bank.cpu().numpy().astype(np.float64)
    sigma = R.scale(hess, 30.0, 1e-2)[2].astype(np.float64)
    zm = np.abs(X.mean(0) - mean) / (sigma / np.sqrt(M))
    zv = np.abs(X.var(0, ddof=1) - sigma ** 2) / (sigma ** 2 * np.sqrt(2.0 / (M - 1)))
    pooled = (((X - mean) / sigma) ** 2).mean()
    print(f"draw law: worst mean at {zm.max():.2f} standard errors, worst variance at {zv.max():.2f}, pooled variance {pooled:.5f}")
    assert (zm <= 6).all() and (zv <= 6).all() and abs(pooled - 1) <= 6 * np.sqrt(2.0 / (P * M))
    assert len(np.unique(X, axis=0)) == M                                        # (every draw is another draw)


# ---------------------------------------------------------------------------------------------- 4. end to end, tiny networks
def _data(dev, mode, n=25):
    g = torch.Generator().manual_seed(5)
    if mode == "classification":
        return torch.randn((n, 1, 4, 4), generator=g).to(dev), torch.randint(0, 3, (n,), generator=g).to(dev)
    x = torch.randn((n, 1), generator=g)
    return x.to(dev), (torch.sin(2 * x) + 0.1 * torch.randn((n, 1), generator=g)).to(dev)


def _state(net, opt):
    d = opt._dev[0]
    return ([p.detach().clone() for p in net.parameters()], [t.clone() for t in d[ivon._MEAN:]], opt.device_step(),
            float(d[ivon._PROD].item()), float(d[ivon._LRW].item()), int(d[ivon._TICKET].abs().sum()), opt._drawn,
            bnn_hip.runtime.state.counter)


def _equal(a, b):
    for x, y in zip(a, b):
        if isinstance(x, list):
            if len(x) != len(y) or not all(torch.equal(s, t) for s, t in zip(x, y)):
                return False
        elif x != y:
            return False
    return True


KW = dict(hess_init=0.5, weight_decay=1e-2, beta2=0.99)
LR, ESS = 0.05, 25.0


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("mode", ["classification", "regression"])
@pytest.mark.parametrize("dropout", [False, True])
def test_tiny_network_end_to_end(dev, mode, dropout, S):
    """5 steps on minibatches of 5: graph replays, eager launches and the epoch runner leave the same bits, and so does a host
    loop opt.perturb(s) / K6's launches / opt.step() -- which also feeds the restated chain with the on-chip noise (materialised)
    and K6's gradients and finds the chain's bits after every step."""
    from bnn_hip import epoch
    X, Y = _data(dev, mode)
    base = _mlp(dev, mode, dropout)
    runs = {}
    for how in ("graph", "eager", "runner", "host"):
        bnn_hip.manual_seed(2026)                                    # (the same dropout masks and draws in every run)
        net = copy.deepcopy(base)
        opt = net.ivon(LR, ESS, samples=S, **KW)
        before = _state(net, opt)
        step = net.graphed_train_step(opt, X[:5], Y[:5], capture=how in ("graph", "runner"))
        assert (step.graph is not None) == (how in ("graph", "runner")) and step.samples == S
        assert step.loss_scale == R.default_loss_scale("cross_entropy" if mode == "classification" else "mse", 5)
        assert _equal(_state(net, opt), before), how                 # building leaves no trace (the snapshot)
        if how == "runner":
            hist = epoch.EpochRunner(step, epoch.DeviceLoader(epoch.DeviceDataset(X, Y), 5, shuffle=False)).run_epoch()
            assert hist.shape == (5, 1) and bool(torch.isfinite(hist).all())
        elif how == "host":
            numels = opt.numels
            ch = R.Chain([p.detach().cpu().numpy() for p in net.parameters()], lr=R.lr_eff(LR, 0.5, 1e-2), ess=ESS, samples=S,
                         loss_scale=step.loss_scale, **KW)
            for j in range(5):
                step.x.copy_(X[5 * j:5 * j + 5].reshape(step.x.shape))
                step.y.copy_(Y[5 * j:5 * j + 5].reshape(step.y.shape))
                opt.sync_lr()
                step._shared.sync()
                step._attach_grads()
                hg = None
                for s in range(S):
                    eps = _device_noise(dev, numels, ch.q(s), opt.seed)[0].cpu().numpy()
                    opt.perturb(s)
                    ch.draw(s, [eps[sl] for sl in ch.sl], hg)
                    assert all(_same(p, c) for p, c in zip(net.parameters(), ch.p)), (j, s)
                    step._enqueue_pass()
                    hg = [p.grad.detach().cpu().numpy().copy() for p in net.parameters()]
                opt.step(loss_scale=step.loss_scale)
                step._shared.advance(S)
                ch.step(hg)
                assert all(_same(p, c) for p, c in zip(net.parameters(), ch.p)), j
                for sl in ch.sl:                                     # (the tensors' slices: the padding is nobody's)
                    assert _same(opt.hess[sl], ch.hess[sl]) and _same(opt.avg_grad[sl], ch.gm[sl]), j
                    assert _same(opt.mean[sl], ch.mean[sl]), j
            assert float(opt._dev[0][ivon._PROD].item()) == ch.prod and ch.t == 5
        else:
            for j in range(5):
                loss = step.step(X[5 * j:5 * j + 5], Y[5 * j:5 * j + 5])
            assert bool(torch.isfinite(loss))
        runs[how] = (net, opt, _state(net, opt), step)
    net, opt, snap, step = runs["graph"]
    for how in ("eager", "runner", "host"):
        assert _equal(snap, runs[how][2]), how
    assert opt.device_step() == 5 and snap[5] == 0 and snap[6] == 0
    assert not torch.equal(opt.hess, torch.full_like(opt.hess, 0.5)) and bool((opt.hess[:opt.numels[0]] > 0).all())
    # the parameters hold the mean between steps: the next step's draw files exactly them
    held = [p.detach().clone() for p in net.parameters()]
    step.step(X[:5], Y[:5])
    assert all(torch.equal(v, h) for v, h in zip(opt._views(opt.mean), held))
    # a further build on a trained optimiser is undone as well
    full = _state(net, opt)
    net.graphed_train_step(opt, X[:5], Y[:5])
    assert _equal(_state(net, opt), full) and full[2] == 6


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("mode", ["classification", "regression"])
def test_step_against_torch_autograd(dev, mode, S):
    """One step in fp32 math without dropout: K6's launches between the draws against torch autograd on the sum loss in their
    place, the same draws (the same seed and step word).  The states agree to the 1e-5 of the largest entry that
    test_gpu_dense_train.py allows K6's fp32 gradients."""
    bnn_hip.set_math("f32")
    X, Y = _data(dev, mode)
    base = _mlp(dev, mode)
    bnn_hip.manual_seed(2026)
    net = copy.deepcopy(base)
    opt = net.ivon(LR, ESS, samples=S, **KW)
    step = net.graphed_train_step(opt, X[:5], Y[:5])
    step.step(X[:5], Y[:5])
    bnn_hip.manual_seed(2026)
    ref = copy.deepcopy(base)
    ropt = ref.ivon(LR, ESS, samples=S, loss_scale=step.loss_scale, **KW)
    for s in range(S):
        ropt.perturb(s)                                               # (s >= 1 folds the gradients of sample s - 1 first)
        ref.zero_grad()
        out = ref(X[:5])
        loss = torch.nn.functional.cross_entropy(out, Y[:5], reduction="sum") if mode == "classification" else \
            torch.nn.functional.mse_loss(out, Y[:5], reduction="sum")
        loss.backward()
    ropt.step()
    assert ropt.device_step() == 1 == opt.device_step()
    for name, got, want in [("param", torch.cat([p.detach().reshape(-1) for p in net.parameters()]),
                             torch.cat([p.detach().reshape(-1) for p in ref.parameters()])),
                            ("hess", opt.hess, ropt.hess), ("avg_grad", opt.avg_grad, ropt.avg_grad)]:
        scale = want.abs().max().item()
        err = (got.double() - want.double()).abs().max().item()
        print(f"{mode} S={S} {name}: max error {err:.3g} against scale {scale:.3g}")
        assert err <= 1e-5 * scale, (name, err, scale)
    assert not torch.equal(opt.avg_grad, torch.zeros_like(opt.avg_grad))


# ---------------------------------------------------------------------------------------------- 5. the posterior
def _trained(dev, mode, steps=5, S=1, ess=400.0):
    X, Y = _data(dev, mode)
    net = _mlp(dev, mode)
    bnn_hip.manual_seed(2026)
    opt = net.ivon(LR, ess, samples=S, **KW)
    step = net.graphed_train_step(opt, X[:5], Y[:5])
    for j in range(steps):
        step.step(X[5 * j:5 * j + 5], Y[5 * j:5 * j + 5])
    return net, opt, step, X, Y


@pytest.mark.parametrize("mode", ["classification", "regression"])
def test_network_and_bank_predictive(dev, mode):
    """network(): mu is the parameters' bits, softplus(rho) the posterior's sigma, the prior N(0, (ess delta)^-1/2).  The bank of
    8 draws and the BayesianNetwork at 8 samples estimate the same predictive mean from independent draws: they agree within
    6 standard errors sqrt(v_bank / 8 + v_net / 8), v the unbiased across-draw variance of each side (classification: of the
    softmax, the network's from 8 single-sample predict_mc calls; regression: the summaries' own), plus 1e-5 for the fp32
    forward.  predict_mc runs in both modes."""
    bnn_hip.set_math("f32")
    net, opt, step, X, Y = _trained(dev, mode)
    bn = opt.network()
    mus = [t for l in (bn.l1, bn.l2, bn.l3) for t in (l.weight_mu, l.bias_mu)]
    rhos = [t for l in (bn.l1, bn.l2, bn.l3) for t in (l.weight_rho, l.bias_rho)]
    for mu, rho, p, v in zip(mus, rhos, net.parameters(), opt.variance()):
        assert torch.equal(mu.data.view(p.shape), p.detach())
        assert torch.allclose(torch.nn.functional.softplus(rho.data.double()).view(p.shape), v.double().sqrt(), rtol=1e-5, atol=0)
    x = X[:5]
    Sn = 8
    bank = opt.sample_bank(Sn)
    assert bank.count() == Sn
    preds, probs = bn.predict_mc(x, 4)                               # (runs in both modes; one class: probabilities of 1)
    assert preds.shape == (5,) and bool(torch.isfinite(probs).all())
    if mode == "classification":
        got = bank.predictive(x).probs
        v_bank = torch.softmax(bank.forward(x), dim=-1).var(dim=0, unbiased=True)
        draws = torch.stack([bn.predict_mc(x, 1)[1] for _ in range(Sn)])          # Sn single draws of the network's softmax
        want, v_net = draws.mean(dim=0), draws.var(dim=0, unbiased=True)
        assert bool(torch.isfinite(bn.predictive(x, Sn).probs).all())
        tol = 6 * torch.sqrt((v_bank + v_net) / Sn) + 1e-5
    else:
        pb, pn = bank.predictive(x, sigma=0.7), bn.predictive(x, Sn, sigma=0.7)
        got, want = pb.mean, pn.mean
        tol = 6 * torch.sqrt((pb.variance + pn.variance) / (Sn - 1)) + 1e-5     # (variance is ddof 0: / (Sn - 1) unbiases it)
    got, want, tol = got.reshape(-1), want.reshape(-1), tol.reshape(-1)
    print(f"{mode}: worst |bank - network| / tolerance = {((got - want).abs() / tol).max().item():.3f}, tolerance up to {tol.max().item():.3g}")
    assert bool(((got - want).abs() <= tol).all())
    assert bank.score(x, Y[:5], sigma=0.7).read().n == 5


# ---------------------------------------------------------------------------------------------- 6. unchanged neighbours
def test_adam_step_enqueues_what_it_did(dev):
    """A FusedAdam step built next to the IVON chain: 3 forward launches, the loss, 3 backward launches and bnn_adam_step, in
    that order and nothing else; 5 graph replays equal 5 eager steps bit for bit.  The IVON chain is 8 S + 1 launches."""
    from bnn_hip.optim import FusedAdam
    X, Y = _data(dev, "classification")
    base = _mlp(dev, "classification", dropout=True)
    out = {}
    for how in ("graph", "eager"):
        bnn_hip.manual_seed(2026)
        net = copy.deepcopy(base)
        opt = FusedAdam(net.parameters(), lr=1e-2, capturable=True)
        step = net.graphed_train_step(opt, X[:5], Y[:5], capture=how == "graph")
        assert step.samples == 1 and not step.ivon
        if how == "eager":
            with L.recording() as calls:
                step.step(X[:5], Y[:5])
            names = [c[2] for c in calls if c[2] != "bnn_stage_inputs"]
            assert names == ["bnn_dense_fwd"] * 3 + ["bnn_dense_loss"] + ["bnn_dense_bwd"] * 3 + ["bnn_adam_step"], names
            first = 1
        else:
            first = 0
        for j in range(first, 5):
            step.step(X[5 * j:5 * j + 5], Y[5 * j:5 * j + 5])
        out[how] = ([p.detach().clone() for p in net.parameters()], bnn_hip.runtime.state.counter)
    assert all(torch.equal(a, b) for a, b in zip(out["graph"][0], out["eager"][0])) and out["graph"][1] == out["eager"][1]
    for S in (1, 3):
        net = copy.deepcopy(base)
        step = net.graphed_train_step(net.ivon(LR, ESS, samples=S, **KW), X[:5], Y[:5], capture=False)
        with L.recording() as calls:
            step.replay()
        names = [c[2] for c in calls]
        one = ["bnn_ivon_draw"] + ["bnn_dense_fwd"] * 3 + ["bnn_dense_loss"] + ["bnn_dense_bwd"] * 3
        assert names == one * S + ["bnn_ivon_step"] and len(names) == 8 * S + 1


# ---------------------------------------------------------------------------------------------- 7. the state dict
@pytest.mark.parametrize("S", [1, 2])
def test_state_dict_round_trip_continues_bit_equal(dev, S):
    """3 steps, the state dict into a fresh optimiser on a copy of the network (loaded in place: the captured step built
    BEFORE the load keeps its addresses), 3 more steps on both: the same bits as the uninterrupted run."""
    net, opt, step, X, Y = _trained(dev, "classification", steps=3, S=S, ess=ESS)
    sd = copy.deepcopy(opt.state_dict())
    assert all(s["step"] == 3 for s in sd["state"].values()) and sd["param_groups"][0]["samples"] == S
    assert all(set(s) == {"hess", "avg_grad", "step"} for s in sd["state"].values())
    net2 = _mlp(dev, "classification", seed=9)
    opt2 = net2.ivon(LR, ESS, samples=S, **KW)
    step2 = net2.graphed_train_step(opt2, X[:5], Y[:5])
    held = [t.data_ptr() for t in opt2._dev[0] if torch.is_tensor(t)]
    net2.load_state_dict(net.state_dict())
    opt2.load_state_dict(sd)
    assert held == [t.data_ptr() for t in opt2._dev[0] if torch.is_tensor(t)]
    assert torch.equal(opt2.hess, opt.hess) and torch.equal(opt2.avg_grad, opt.avg_grad) and opt2.device_step() == 3
    assert float(opt2._dev[0][ivon._PROD].item()) == float(opt._dev[0][ivon._PROD].item()) == 0.9 * 0.9 * 0.9
    for p in net2.parameters():
        assert opt2.state[p]["hess"].data_ptr() >= opt2.hess.data_ptr() and opt2.state[p]["hess"].shape == p.shape
    counter = bnn_hip.runtime.state.counter
    for j in range(3, 5):
        step.step(X[5 * j:5 * j + 5], Y[5 * j:5 * j + 5])
    bnn_hip.runtime.state.counter = counter                          # (the same sample indices for the second run)
    for j in range(3, 5):
        step2.step(X[5 * j:5 * j + 5], Y[5 * j:5 * j + 5])
    assert all(torch.equal(a, b) for a, b in zip(net.parameters(), net2.parameters()))
    assert torch.equal(opt2.hess, opt.hess) and torch.equal(opt2.avg_grad, opt.avg_grad) and opt2.device_step() == 5
    # a scheduler's rate reaches the captured step through the device word, rescaled
    opt.param_groups[0]["lr"] = 0.01
    step.step(X[:5], Y[:5])
    assert float(opt._dev[0][ivon._LRW].item()) == float(np.float32(0.01 * (0.5 + 1e-2)))


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals(dev):
    import networks
    from bnn_hip.ensemble import EnsembleTrainStep
    X, Y = _data(dev, "classification")
    net = _mlp(dev, "classification")
    opt = net.ivon(0.1, 100.0)
    with pytest.raises(BnnHipError, match="FusedIVON is not supported"):
        EnsembleTrainStep(net.ensemble(2, seeds=range(2)), opt, X[:5], Y[:5])
    ps = list(net.parameters())
    with pytest.raises(BnnHipError, match="one group"):
        ivon.FusedIVON([dict(params=ps[:2]), dict(params=ps[2:])], 0.1, 100.0)
    with pytest.raises(BnnHipError, match="samples"):
        net.ivon(0.1, 100.0, samples=9)
    mp = dict(input_shape=16, classes=3, batch_size=5, hidden_units=8, mode="classification", mu_init=[-0.2, 0.2],
              rho_init=[-5.0, -4.0], prior_init=[1.0], mixture_prior=False, local_reparam=False)
    bbb = networks.BayesianNetwork(mp).to(dev)
    assert not hasattr(bbb, "ivon")
    with pytest.raises(BnnHipError, match="BBB"):                    # a BBB network is not K6's stack of Linear layers
        ivon.FusedIVON(bbb.parameters(), 0.1, 100.0, mlp=bbb)
    with pytest.raises(BnnHipError, match="BBB"):
        networks.MLP.graphed_train_step(bbb, ivon.FusedIVON(bbb.parameters(), 0.1, 100.0), X[:5], Y[:5])
    with pytest.raises(BnnHipError, match="needs the network"):
        ivon.FusedIVON(ps, 0.1, 100.0).sample_bank(3)
    with pytest.raises(BnnHipError, match="layer order"):
        ivon.FusedIVON(ps[::-1], 0.1, 100.0, mlp=net).network()
    with pytest.raises(BnnHipError, match="capturable"):
        net.graphed_train_step(net.ivon(0.1, 100.0, capturable=False), X[:5], Y[:5])
    # step() before perturb(), a draw out of order, posterior access inside a step
    for p in ps:
        p.grad = torch.zeros_like(p)
    with pytest.raises(BnnHipError, match="perturb"):
        opt.step(loss_scale=1.0)
    opt.perturb(0)
    with pytest.raises(BnnHipError, match="out of order"):
        opt.perturb(0)
    with pytest.raises(BnnHipError, match="under way"):
        opt.sample_bank(3)
    with pytest.raises(BnnHipError, match="under way"):
        net.graphed_train_step(opt, X[:5], Y[:5])
    with pytest.raises(BnnHipError, match="loss_scale is unresolved"):
        opt.step()
    opt.step(loss_scale=1.0)
    assert opt.device_step() == 1 and opt.sample_bank(3, sample_offset=0).count() == 3
    other = _mlp(dev, "regression")
    with pytest.raises(BnnHipError, match="parameter shapes"):
        opt.sample_bank(3, other.weight_bank(3))
    for p in ps:
        p.grad = None
    opt.perturb(0)
    with pytest.raises(BnnHipError, match="gradient"):
        opt.step(loss_scale=1.0)
