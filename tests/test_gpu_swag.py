"""SWAG on an MI355X (bnn_swag_step / bnn_swag_sample, bnn_hip.swag; include/bnn_hip.h F22) against the numpy restatement
(tests/swag_ref.py): the step, the moments and the ring bit for bit, the step against FusedSGD's bits and torch.optim.SGD, the
moments against fp64, the draw bit for bit on given noise and on the materialised on-chip streams, its chunking and its law, and
tiny networks fitted end to end (graph replays, eager launches, the epoch runner and a plain FusedSGD run give the same bits)."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bnn_hip
import optim_ref as O
import swag_ref as R
from bnn_hip import _lib as L
from bnn_hip import ops, sgmcmc, swag
from bnn_hip.ops import BnnHipError

SEED = 0x5EED0123456789AB
NUMELS = (1, 5, 37, 1201, 4096, 4100)   # one element, a tail below 4, odd tails, an exact chunk, a chunk plus one float4
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


def _words(dev, step=0, count=0):
    return sgmcmc._word(step, dev), sgmcmc._word(count, dev), torch.zeros(16, dtype=torch.int32, device=dev)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _same(got, want):
    return np.array_equal(_bits(got).reshape(-1), np.ascontiguousarray(want, dtype=np.float32).view(np.uint32).reshape(-1))


def _tensors(dev, numels, seed, scale=1.0, shift=0.0):
    rng = np.random.default_rng(seed)
    host = [(shift + rng.standard_normal(n) * scale).astype(np.float32) for n in numels]
    return host, [torch.from_numpy(h).to(dev) for h in host]


def _moment_buffers(numels, K, fill=0.0):
    """(mean, m2, dev) host arrays: `fill` where the tensors live, the sentinel in the padding."""
    offs, stride = R.layout(list(numels))
    out = []
    for rows in (None, None, K):
        a = np.full(stride if rows is None else (rows, stride), SENTINEL, dtype=np.float32)
        for o, n in zip(offs, numels):
            a[..., o:o + n] = fill
        out.append(a)
    return out[0], out[1], (out[2] if K else None)


def _to(dev, a):
    return None if a is None else torch.from_numpy(a.copy()).to(dev)


# ---------------------------------------------------------------------------------------------- 1. the step, bit for bit
@pytest.mark.parametrize("K", [0, 2, 3, 32])
@pytest.mark.parametrize("momentum", [False, True])
@pytest.mark.parametrize("wd", [0.0, 1e-3])
def test_step_bit_for_bit(dev, K, momentum, wd):
    """start 2, every 1, K + 4 launches over the six tensors: two steps that do not collect, then counts 0 .. K + 1 -- n = 0, 1,
    K - 1, K and K + 1, so the ring wraps.  After every launch the parameters, the momenta, the moments, the ring (padding
    included: the sentinel) and the three words are the restated chain's."""
    lr, mu = 0.05, 0.9
    hp, dp = _tensors(dev, NUMELS, 1, 0.3)
    hmean, hm2, hdev = _moment_buffers(NUMELS, K)
    dmean, dm2, ddev = _to(dev, hmean), _to(dev, hm2), _to(dev, hdev)
    dm = [torch.zeros_like(p) for p in dp] if momentum else None
    ch = R.Chain(hp, lr=lr, mu=mu, wd=wd, momentum=momentum, start=2, every=1, rank=K, mean=hmean, m2=hm2, dev=hdev)
    step, count, ticket = _words(dev)
    lr_dev = torch.tensor([lr], dtype=torch.float32, device=dev) if momentum else None     # (both ways of passing the rate)
    for k in range(K + 4):
        hg, dg = _tensors(dev, NUMELS, 10 + k, 0.05)
        ch.step(hg)
        ops.swag_step(dp, dg, lr=lr if lr_dev is None else 123.0, momentum=mu, weight_decay=wd, lr_device=lr_dev, momenta=dm,
                      start=2, every=1, mean=dmean, m2=dm2, dev=ddev, step=step, count=count, ticket=ticket)
        for t in range(len(NUMELS)):
            assert _same(dp[t], ch.p[t]), (k, t)
            assert not momentum or _same(dm[t], ch.v[t]), (k, t)
        assert _same(dmean, hmean) and _same(dm2, hm2), k
        assert K == 0 or _same(ddev, hdev), k
        assert sgmcmc._read_word(step) == k + 1 == ch.k and sgmcmc._read_word(count) == max(0, k - 1) == ch.n
        assert int(ticket.abs().sum()) == 0
    assert ch.collected_at == list(range(2, K + 4))
    if K:
        assert not np.isin(SENTINEL, hdev[:, :1]) and (hdev[:, 1:64] == SENTINEL).all()      # (every row written, no padding)


@pytest.mark.parametrize("blocks", sorted(O.GRIDS))
@pytest.mark.parametrize("momentum", [False, True])
def test_step_bit_for_bit_at_every_grid(dev, blocks, momentum):
    """The launch's last block (csrc/bnn_stream.h: 8 ticket groups, then word 0) at grids of 1, 2, 7, 8, 9, 16 and 17 blocks.
    Three launches, start 1, every 1, rank 2 (one launch that does not collect, two that do): after every launch the
    parameters, the momenta, the moments and the ring are the restated chain's, the step word has advanced by exactly one, the
    count word is the chain's and every ticket word is zero."""
    numels = O.GRIDS[blocks]
    assert len(O.chunk_table(numels)) == blocks
    lr, mu, wd, K = 0.05, 0.9, 1e-3, 2
    hp, dp = _tensors(dev, numels, 1, 0.3)
    hmean, hm2, hdev = _moment_buffers(numels, K)
    dmean, dm2, ddev = _to(dev, hmean), _to(dev, hm2), _to(dev, hdev)
    dm = [torch.zeros_like(p) for p in dp] if momentum else None
    ch = R.Chain(hp, lr=lr, mu=mu, wd=wd, momentum=momentum, start=1, every=1, rank=K, mean=hmean, m2=hm2, dev=hdev)
    step, count, ticket = _words(dev)
    for k in range(3):
        hg, dg = _tensors(dev, numels, 10 + k, 0.05)
        ch.step(hg)
        ops.swag_step(dp, dg, lr=lr, momentum=mu, weight_decay=wd, momenta=dm, start=1, every=1, mean=dmean, m2=dm2, dev=ddev,
                      step=step, count=count, ticket=ticket)
        for t in range(len(numels)):
            assert _same(dp[t], ch.p[t]), (k, t)
            assert not momentum or _same(dm[t], ch.v[t]), (k, t)
        assert _same(dmean, hmean) and _same(dm2, hm2) and _same(ddev, hdev), k
        assert sgmcmc._read_word(step) == k + 1 == ch.k and sgmcmc._read_word(count) == k == ch.n, k
        assert not ticket.any(), k
    assert ch.collected_at == [1, 2]


def test_step_with_sixteen_tensors(dev):
    numels = (3, 64, 65, 130, 7, 1, 4096, 4097, 12, 255, 256, 257, 1023, 2, 5000, 33)
    assert len(numels) == L.SGMCMC_MAX_TENSORS
    hp, dp = _tensors(dev, numels, 2, 0.3)
    hmean, hm2, hdev = _moment_buffers(numels, 2, fill=0.25)
    dmean, dm2, ddev = _to(dev, hmean), _to(dev, hm2), _to(dev, hdev)
    dm = [torch.zeros_like(p) for p in dp]
    ch = R.Chain(hp, lr=0.02, mu=0.5, wd=1e-2, momentum=True, start=0, every=1, rank=2, count=3, step=9, mean=hmean, m2=hm2, dev=hdev)
    step, count, ticket = _words(dev, 9, 3)
    for k in range(2):
        hg, dg = _tensors(dev, numels, 30 + k, 0.05)
        ch.step(hg)
        ops.swag_step(dp, dg, lr=0.02, momentum=0.5, weight_decay=1e-2, momenta=dm, mean=dmean, m2=dm2, dev=ddev, step=step,
                      count=count, ticket=ticket)
    for t in range(len(numels)):
        assert _same(dp[t], ch.p[t]) and _same(dm[t], ch.v[t]), t
    assert _same(dmean, hmean) and _same(dm2, hm2) and _same(ddev, hdev)
    assert sgmcmc._read_word(step) == 11 and sgmcmc._read_word(count) == 5 and int(ticket.abs().sum()) == 0


# ---------------------------------------------------------------------------------------------- 2. against FusedSGD
@pytest.mark.parametrize("wd", [0.0, 1e-3])
def test_step_without_momentum_is_sgd_step_bit_for_bit(dev, wd):
    _, dp = _tensors(dev, NUMELS, 3, 0.3)
    _, dg = _tensors(dev, NUMELS, 4, 0.05)
    want = [p.clone() for p in dp]
    lr_dev = torch.tensor([0.0371], dtype=torch.float32, device=dev)
    ops.sgd_step(want, dg, lr=9.0, weight_decay=wd, lr_device=lr_dev)
    hmean, hm2, hdev = _moment_buffers(NUMELS, 3, fill=0.5)
    dmean, dm2, ddev = _to(dev, hmean), _to(dev, hm2), _to(dev, hdev)
    step, count, ticket = _words(dev)
    ops.swag_step(dp, dg, lr=9.0, weight_decay=wd, lr_device=lr_dev, start=5, every=1, mean=dmean, m2=dm2, dev=ddev, step=step,
                  count=count, ticket=ticket)
    assert all(torch.equal(a, b) for a, b in zip(dp, want))
    # nothing collected: the moments are untouched, the step word moved
    assert _same(dmean, hmean) and _same(dm2, hm2) and _same(ddev, hdev)
    assert sgmcmc._read_word(step) == 1 and sgmcmc._read_word(count) == 0


# ---------------------------------------------------------------------------------------------- 3. against torch.optim.SGD
def test_step_against_torch_sgd_with_momentum(dev):
    """Three steps of torch.optim.SGD(momentum 0.9, weight_decay 1e-3) on the same device.  The two compute the same recursion
    g' = g + wd p, v' = mu v + g', p' = p - lr v'; the kernel rounds each line once (one fma), torch's unfused form at most
    twice (product, then sum).  With u = 2^-24 and G, V, P the largest |g'|, |v|, |p| met, one step separates the two by
    at most  dg <= 3 u G,  dv' <= mu dv + dg + 3 u V,  dp' <= (1 + lr wd) dp + lr dv' + 3 u P  (one rounding of ours plus two of
    torch's per line, the earlier differences carried through the exact recursion): iterated three times from 0 that is a few
    ulp of the largest magnitude."""
    lr, mu, wd, u = 0.05, 0.9, 1e-3, 2.0 ** -24
    hp, dp = _tensors(dev, NUMELS, 5, 1.0)
    tp = [torch.nn.Parameter(p.clone()) for p in dp]
    topt = torch.optim.SGD(tp, lr=lr, momentum=mu, weight_decay=wd)
    dm = [torch.zeros_like(p) for p in dp]
    hmean, hm2, hdev = _moment_buffers(NUMELS, 0)
    dmean, dm2 = _to(dev, hmean), _to(dev, hm2)
    step, count, ticket = _words(dev)
    G = V = 0.0
    P = max(float(p.abs().max()) for p in dp)
    dv = dpb = 0.0
    for k in range(3):
        _, dg = _tensors(dev, NUMELS, 50 + k, 0.5)
        G = max(G, max(float((g.abs() + wd * p.abs()).max()) for g, p in zip(dg, dp)))
        for p, g in zip(tp, dg):
            p.grad = g.clone()
        topt.step()
        ops.swag_step(dp, dg, lr=lr, momentum=mu, weight_decay=wd, momenta=dm, start=100, mean=dmean, m2=dm2, dev=None, step=step,
                      count=count, ticket=ticket)
        V = max(V, max(float(m.abs().max()) for m in dm))
        P = max(P, max(float(p.abs().max()) for p in dp))
        dv = mu * dv + 3 * u * G + 3 * u * V
        dpb = (1 + lr * wd) * dpb + lr * dv + 3 * u * P
        err_p = max(float((a - b.detach()).abs().max()) for a, b in zip(dp, tp))
        err_v = max(float((a - topt.state[b]["momentum_buffer"]).abs().max()) for a, b in zip(dm, tp))
        print(f"step {k}: |p - torch| = {err_p:.3e} (bound {dpb:.3e}), |v - torch| = {err_v:.3e} (bound {dv:.3e})")
        assert err_p <= dpb and err_v <= dv, k
    assert dpb <= 16 * u * P                                         # "a few ulp of the largest magnitude"


# ---------------------------------------------------------------------------------------------- 4. the moments against fp64
def test_moments_against_fp64(dev):
    """8 collected iterates near 1 with spread 1e-3 (kappa = |mean| / sigma ~ 1e3; the two-moment form mean(x^2) - mean(x)^2
    would lose kappa^2 u ~ 6 % in fp32).  Welford's update here: d_k = p_k - mean_{k-1} is exact given the computed mean
    (Sterbenz), and the computed mean is off by at most k u |mean| after k roundings, so every d and d' is off by at most
    n u |mean|; with sum_k (|d_k| + |d'_k|) <= 2 sqrt(2 n S) (Cauchy-Schwarz, sum d_k^2 <= 2 S) and one rounding per accumulation
    (n u S) the relative error of S = m2 is at most 2 sqrt(2) n u kappa + n u.  Asserted per element with its own kappa:
    |m2 / n - var| <= n u (3 kappa + 2) var (3 >= 2 sqrt 2; + 2: the accumulation and the final division by n)."""
    n, u = 8, 2.0 ** -24
    numels = (37, 1201)
    _, dp = _tensors(dev, numels, 6, 1e-3, shift=1.0)
    hmean, hm2, _ = _moment_buffers(numels, 0)
    dmean, dm2 = _to(dev, hmean), _to(dev, hm2)
    step, count, ticket = _words(dev)
    its = []
    for k in range(n):
        _, dg = _tensors(dev, numels, 70 + k, 1e-3)
        ops.swag_step(dp, dg, lr=1.0, mean=dmean, m2=dm2, dev=None, step=step, count=count, ticket=ticket)
        its.append([p.cpu().numpy().astype(np.float64) for p in dp])
    assert sgmcmc._read_word(count) == n
    offs, _ = R.layout(list(numels))
    worst = 0.0
    for t, (o, m) in enumerate(zip(offs, numels)):
        X = np.stack([it[t] for it in its])
        var, mean = X.var(axis=0), X.mean(axis=0)
        got = dm2[o:o + m].cpu().numpy().astype(np.float64) / n
        kappa = np.abs(mean) / np.sqrt(var)
        bound = n * u * (3 * kappa + 2) * var
        worst = max(worst, float((np.abs(got - var) / bound).max()))
        assert (np.abs(got - var) <= bound).all(), (t, worst)
        assert np.abs(dmean[o:o + m].cpu().numpy() - mean).max() <= 2 * n * u * np.abs(mean).max()
        assert kappa.min() > 100                                     # (the regime the bound is about)
    print(f"m2 / n against the fp64 variance: worst error / bound = {worst:.3f}")


# ---------------------------------------------------------------------------------------------- 5. the draw, bit for bit
def _posterior_arrays(numels, K, n, seed):
    """Moments as a collector leaves them after n iterates: the rows of D not written yet (>= min(n, K)) hold NaN, and so
    prove that the draw does not read them; the padding holds the sentinel."""
    rng = np.random.default_rng(seed)
    offs, stride = R.layout(list(numels))
    mean, m2, dev = _moment_buffers(numels, K)
    for o, m in zip(offs, numels):
        mean[o:o + m] = rng.standard_normal(m)
        m2[o:o + m] = n * 10.0 ** rng.uniform(-6, 0, m)
        m2[o] = 0.0                                                  # (the variance clamp)
        for j in range(K):
            dev[j, o:o + m] = 0.1 * rng.standard_normal(m) if j < min(n, K) else np.nan
    return mean, m2, dev


def _ref_members(numels, mean, m2, dev, n, z1, z2, **kw):
    """[m, stride]: the restated draw per member over the tensors' elements; NaN elsewhere (never compared)."""
    offs, stride = R.layout(list(numels))
    out = np.full((z1.shape[0], stride), np.nan, dtype=np.float32)
    for q in range(z1.shape[0]):
        for o, m in zip(offs, numels):
            sl = slice(o, o + m)
            out[q, sl] = R.draw(mean[sl], m2[sl], None if dev is None else dev[:, sl], n, z1[q, sl],
                                None if z2 is None else z2[q], **kw)
    return out


def _check_bank(bank, hbank0, want, numels, first):
    """Members [first, first + m) equal `want` on the tensors' elements; every other word of the bank is as it was."""
    offs, stride = R.layout(list(numels))
    got = bank.cpu().numpy()
    keep = np.ones(got.shape, dtype=bool)
    for o, m in zip(offs, numels):
        sl = slice(o, o + m)
        blk = got[first:first + want.shape[0], sl]
        assert np.array_equal(blk.view(np.uint32), want[:, sl].view(np.uint32)), (o, m)
        keep[first:first + want.shape[0], sl] = False
    assert np.array_equal(got[keep].view(np.uint32), hbank0[keep].view(np.uint32))


@pytest.mark.parametrize("K", [2, 3, 32])
@pytest.mark.parametrize("low_rank", [True, False])
def test_draw_on_given_noise_bit_for_bit(dev, K, low_rank):
    """BNN_EPS_MEMORY against the restatement over n in {2, K, K + 1}, m in {1, 3, 9}, first in {0, 2}; members outside
    [first, first + m) and the padding keep the sentinel; BNN_EPS_ZERO gives the mean's bits."""
    offs, stride = R.layout(list(NUMELS))
    rng = np.random.default_rng(K)
    for n in sorted({2, K, K + 1}):
        mean, m2, hdev = _posterior_arrays(NUMELS, K, n, seed=100 + n)
        dmean, dm2, ddev = _to(dev, mean), _to(dev, m2), _to(dev, hdev)
        count = sgmcmc._word(n, dev)
        for m in (1, 3, 9):
            for first in (0, 2):
                z1 = rng.standard_normal((m, stride)).astype(np.float32)
                z2 = rng.standard_normal((m, K)).astype(np.float32)
                hbank0 = np.full((12, stride), SENTINEL, dtype=np.float32)
                bank = _to(dev, hbank0)
                kw = dict(scale=0.7, low_rank=low_rank, var_clamp=1e-8)
                ops.swag_sample(NUMELS, dmean, dm2, ddev, count, bank, members=m, first=first, eps_mode=L.EPS_MEMORY,
                                z1=_to(dev, z1), z2=_to(dev, z2) if low_rank else None, **kw)
                want = _ref_members(NUMELS, mean, m2, hdev, n, z1, z2 if low_rank else None, **kw)
                _check_bank(bank, hbank0, want, NUMELS, first)
                assert np.isfinite(want[:, offs[2]:offs[2] + 37]).all()
        bank = _to(dev, hbank0)
        ops.swag_sample(NUMELS, dmean, dm2, ddev, count, bank, members=3, first=1, eps_mode=L.EPS_ZERO, low_rank=low_rank)
        _check_bank(bank, hbank0, np.broadcast_to(mean, (3, stride)).copy(), NUMELS, 1)


def _device_streams(dev, numels, K, base, m):
    """(z1 [m, stride], z2 [m, K]) of draws base .. base + m - 1, materialised through the sampler itself.  z1: mean 0, m2 = n
    = 4 (m2 / n = 1 exactly), SWAG-Diagonal at scale 1 (c_d = 1): theta = fma(1, z1, 0) = z1.  z2: one tensor of 64 elements,
    D[j][j] = 1, m2 = 0 at var_clamp 0 (s = 0), scale = 2 (K - 1) so that c_lr[K] = 1: theta[j] = fma(1, z2[j], fma(0, z1, 0))."""
    _, stride = R.layout(list(numels))
    zero = torch.zeros(stride, device=dev)
    z1 = torch.zeros((m, stride), device=dev)
    ops.swag_sample(numels, zero, torch.full((stride,), 4.0, device=dev), None, sgmcmc._word(4, dev), z1, members=m, scale=1.0,
                    low_rank=False, seed=SEED, sample_base=base)
    eye = torch.zeros((K, 64), device=dev)
    eye[torch.arange(K), torch.arange(K)] = 1.0
    z2 = torch.zeros((m, 64), device=dev)
    ops.swag_sample([64], torch.zeros(64, device=dev), torch.zeros(64, device=dev), eye, sgmcmc._word(K, dev), z2, members=m,
                    scale=2.0 * (K - 1), var_clamp=0.0, seed=SEED, sample_base=base)
    assert bool((z2[:, K:] == 0).all())
    return z1, z2[:, :K].contiguous()


@pytest.mark.parametrize("K", [2, 3, 32])
def test_draw_on_the_chip_streams(dev, K):
    """BNN_EPS_PHILOX: the two streams, materialised through the sampler, are the restated streams (to the 5e-5 the device's
    transcendentals allow, as every stream here), pure functions of (seed, q, t, i) / (seed, q, j); the Philox draw equals the
    restated draw on the materialised noise bit for bit, and so the memory-mode draw on it."""
    offs, stride = R.layout(list(NUMELS))
    base, m = 2 ** 32 - 2, 5                                         # (the draw index wraps as a 32-bit word)
    z1, z2 = _device_streams(dev, NUMELS, K, base, m)
    for q in range(m):
        for t, (o, n) in enumerate(zip(offs, NUMELS)):
            np.testing.assert_allclose(z1[q, o:o + n].cpu().numpy(), R.z1(SEED, base + q, t, n), atol=5e-5, rtol=0)
        np.testing.assert_allclose(z2[q].cpu().numpy(), R.z2(SEED, base + q, K), atol=5e-5, rtol=0)
    # purity: a launch of one member at another place of the draw, other neighbours in the tensor list, another rank
    one1, one2 = _device_streams(dev, NUMELS[:3], max(2, K - 1), base + 3, 1)
    assert torch.equal(one1[0, :offs[2] + 37], z1[3, :offs[2] + 37]) and torch.equal(one2[0], z2[3, :max(2, K - 1)])
    hz1, hz2 = z1.cpu().numpy(), z2.cpu().numpy()
    for n in sorted({2, K, K + 1}):
        mean, m2, hdev = _posterior_arrays(NUMELS, K, n, seed=200 + n)
        dmean, dm2, ddev = _to(dev, mean), _to(dev, m2), _to(dev, hdev)
        count = sgmcmc._word(n, dev)
        for low_rank in (True, False):
            hbank0 = np.full((8, stride), SENTINEL, dtype=np.float32)
            bank, bank_mem = _to(dev, hbank0), _to(dev, hbank0)
            kw = dict(scale=1.3, low_rank=low_rank, var_clamp=1e-8)
            ops.swag_sample(NUMELS, dmean, dm2, ddev, count, bank, members=m, first=2, seed=SEED, sample_base=base, **kw)
            want = _ref_members(NUMELS, mean, m2, hdev, n, hz1, hz2 if low_rank else None, **kw)
            _check_bank(bank, hbank0, want, NUMELS, 2)
            ops.swag_sample(NUMELS, dmean, dm2, ddev, count, bank_mem, members=m, first=2, eps_mode=L.EPS_MEMORY, z1=z1,
                            z2=z2 if low_rank else None, **kw)
            assert torch.equal(bank, bank_mem)


# ---------------------------------------------------------------------------------------------- 6. chunking, determinism
def _mlp(dev, mode, dropout=False, seed=0):
    import networks
    torch.manual_seed(seed)
    if mode == "classification":
        mp = dict(input_shape=16, classes=3, batch_size=5, hidden_units=8, mode=mode)
    else:
        mp = dict(input_shape=1, classes=1, batch_size=5, hidden_units=40, mode=mode)
    return (networks.MLP_Dropout if dropout else networks.MLP)(mp).to(dev)


def _filled_posterior(dev, rank=3, n=5):
    net = _mlp(dev, "classification")
    post = swag.SwagPosterior(net, rank=rank)
    g = torch.Generator().manual_seed(3)
    post.mean.copy_(torch.randn(post.stride, generator=g))
    post.m2.copy_(n * 0.01 * torch.rand(post.stride, generator=g))
    if rank:
        post.dev.copy_(0.05 * torch.randn((rank, post.stride), generator=g))
    sgmcmc._set_word(post.count_word, n)
    return net, post


def test_sample_bank_chunking_and_determinism(dev):
    net, post = _filled_posterior(dev)
    bnn_hip.manual_seed(11, counter=40)
    a = post.sample_bank(5, sample_offset=100)
    b = post.sample_bank(5, sample_offset=100, members_per_launch=1)
    c = post.sample_bank(5, sample_offset=100, members_per_launch=2)
    assert torch.equal(a.buffer, b.buffer) and torch.equal(a.buffer, c.buffer) and a.count() == 5 and a.capacity == 5
    d = post.sample_bank(5, sample_offset=105)
    assert not torch.equal(a.buffer, d.buffer) and torch.equal(post.sample_bank(7, sample_offset=100).buffer[5:], d.buffer[:2])
    assert bnn_hip.runtime.state.counter == 40                        # (an explicit offset takes nothing from the counter)
    e = post.sample_bank(3)
    assert bnn_hip.runtime.state.counter == 43 and torch.equal(e.buffer, post.sample_bank(3, sample_offset=40).buffer)
    # KronLaplace.sample_bank's contract: a bank passed in keeps a higher `collected`, a lower one is raised
    big = net.weight_bank(8)
    sgmcmc._set_word(big.collected, 7)
    assert post.sample_bank(5, big, sample_offset=100) is big and sgmcmc._read_word(big.collected) == 7
    assert torch.equal(big.buffer[:5], a.buffer) and not big.buffer[5:].any()
    small = net.weight_bank(8)
    post.sample_bank(5, small, sample_offset=100)
    assert small.count() == 5
    # SWAG-Diagonal draws are other draws of the same mean
    diag = post.sample_bank(5, sample_offset=100, low_rank=False)
    assert not torch.equal(diag.buffer, a.buffer)
    bnn_hip.manual_seed(12)
    assert not torch.equal(post.sample_bank(5, sample_offset=100).buffer, a.buffer)          # (the seed keys the streams)


# ---------------------------------------------------------------------------------------------- 7. the law of the draw
def test_draw_law(dev):
    """One tensor of 37 elements, K = 3, 4096 draws (64 launches of 64 members): the sample mean within 6 standard errors
    sqrt(S_ii / M) of the mean and the sample covariance within 6 sqrt((S_ii S_jj + S_ij^2) / M) of the exact covariance
    (tests/swag_ref.covariance, fp64), entry by entry."""
    P, K, n, M = 37, 3, 5, 4096
    rng = np.random.default_rng(8)
    mean = rng.standard_normal(64).astype(np.float32)
    m2 = (n * rng.uniform(0.5, 2.0, 64)).astype(np.float32)
    hdev = (0.8 * rng.standard_normal((K, 64))).astype(np.float32)
    bank = torch.zeros((M, 64), device=dev)
    for first in range(0, M, L.SWAG_MAX_MEMBERS):
        ops.swag_sample([P], _to(dev, mean), _to(dev, m2), _to(dev, hdev), sgmcmc._word(n, dev), bank, members=L.SWAG_MAX_MEMBERS,
                        first=first, scale=0.9, seed=SEED, sample_base=first)
    X = bank[:, :P].cpu().numpy().astype(np.float64)
    assert not bank[:, P:].any()
    S = R.covariance(m2[:P], hdev[:, :P], n, scale=0.9)
    np.testing.assert_allclose(S, R.swag_covariance(m2[:P].astype(np.float64) / n, hdev[:, :P], K, 0.9), rtol=1e-6)
    sd = np.sqrt(np.diag(S))
    assert (np.abs(X.mean(0) - mean[:P]) <= 6 * sd / np.sqrt(M)).all()
    C = np.cov(X, rowvar=False)
    se = np.sqrt((np.outer(np.diag(S), np.diag(S)) + S * S) / M)
    z = np.abs(C - S) / se
    print(f"draw law: worst covariance entry at {z.max():.2f} standard errors, off-diagonal mass {np.abs(S - np.diag(np.diag(S))).sum():.2f}")
    assert (z <= 6).all()
    assert np.abs(S - np.diag(np.diag(S))).max() > 5 * se.max()      # (the low-rank term is visible at this M)


# ---------------------------------------------------------------------------------------------- 8. end to end, tiny networks
def _data(dev, mode, n=60):
    g = torch.Generator().manual_seed(5)
    if mode == "classification":
        return torch.randn((n, 1, 4, 4), generator=g).to(dev), torch.randint(0, 3, (n,), generator=g).to(dev)
    x = torch.randn((n, 1), generator=g)
    return x.to(dev), (torch.sin(2 * x) + 0.1 * torch.randn((n, 1), generator=g)).to(dev)


def _state(net, opt, post):
    mom = [opt.state[p]["momentum_buffer"].clone() for p in net.parameters() if "momentum_buffer" in opt.state.get(p, {})]
    return ([p.detach().clone() for p in net.parameters()], mom, post.mean.clone(), post.m2.clone(),
            None if post.dev is None else post.dev.clone(), post.count(), opt.device_step(), float(opt._dev[0][0]))


def _equal(a, b):
    for x, y in zip(a, b):
        if isinstance(x, list):
            if len(x) != len(y) or not all(torch.equal(s, t) for s, t in zip(x, y)):
                return False
        elif torch.is_tensor(x):
            if not torch.equal(x, y):
                return False
        elif x != y:
            return False
    return True


LR, WD = 0.02, 1e-3


@pytest.mark.parametrize("mode", ["classification", "regression"])
@pytest.mark.parametrize("dropout", [False, True])
def test_tiny_network_end_to_end(dev, mode, dropout):
    from bnn_hip import epoch
    from bnn_hip.optim import FusedSGD
    X, Y = _data(dev, mode)
    base = _mlp(dev, mode, dropout)
    runs = {}
    for how in ("graph", "eager", "runner", "sgd"):
        bnn_hip.manual_seed(2026)                                    # (the same dropout masks in every run)
        net = copy.deepcopy(base)
        if how == "sgd":
            opt = FusedSGD(net.parameters(), LR, weight_decay=WD, capturable=True)
            step = net.graphed_train_step(opt, X[:5], Y[:5])
            its = []
            for j in range(12):
                step.step(X[5 * j:5 * j + 5], Y[5 * j:5 * j + 5])
                its.append([p.detach().cpu().numpy().copy() for p in net.parameters()])
            runs[how] = its
            continue
        opt, post = net.swag(LR, weight_decay=WD, start=4, every=2, rank=3)
        before = _state(net, opt, post)
        step = net.graphed_train_step(opt, X[:5], Y[:5], capture=how != "eager")
        assert (step.graph is not None) == (how != "eager")
        assert _equal(_state(net, opt, post), before), how           # building leaves no trace
        if how == "runner":
            hist = epoch.EpochRunner(step, epoch.DeviceLoader(epoch.DeviceDataset(X, Y), 5, shuffle=False)).run_epoch()
            assert hist.shape == (12, 1) and bool(torch.isfinite(hist).all())
        else:
            for j in range(12):
                loss = step.step(X[5 * j:5 * j + 5], Y[5 * j:5 * j + 5])
            assert bool(torch.isfinite(loss))
        runs[how] = (net, opt, post, _state(net, opt, post), step)
    net, opt, post, snap, step = runs["graph"]
    assert _equal(snap, runs["eager"][3]) and _equal(snap, runs["runner"][3])
    assert post.count() == 4 and opt.device_step() == 12 and int(opt._dev[0][swag._TICKET].abs().sum()) == 0
    # the iterates are a plain FusedSGD run's; the moments are the restated chain fed with its iterates 5, 7, 9, 11
    its = runs["sgd"]
    assert all(np.array_equal(a, p.detach().cpu().numpy()) for a, p in zip(its[11], net.parameters()))
    ch = R.Chain([np.zeros(s, np.float32) for s in post.shapes], lr=LR, rank=3)
    for k in (5, 7, 9, 11):
        ch.collect(its[k])
    assert _same(post.mean, ch.mean) and _same(post.m2, ch.m2) and _same(post.dev, ch.dev)
    for v, w in zip(post.variance(), post.mean_views()):
        assert v.shape == w.shape and bool((v >= 0).all())
    assert tuple(post.variance()[0].shape) == post.shapes[0]

    # a further step on a built posterior: building again (the warm-up collects at step word 13) is undone
    step.step(X[:5], Y[:5])
    full = _state(net, opt, post)
    assert full[5] == 4 and full[6] == 13
    net.graphed_train_step(opt, X[:5], Y[:5])
    assert _equal(_state(net, opt, post), full)

    # full SWAG through the bank's launches, and a predictive captured BEFORE the bank is re-sampled
    x, y = X[:5], Y[:5]
    kw = dict(quantiles=[0.1, 0.9]) if mode == "regression" else {}
    bank = post.sample_bank(5, sample_offset=0)
    assert bank.count() == 5 and bank.capacity == 5
    graphed = bank.predictive_graph(x, sigma=0.7, **kw)
    first_mean = graphed.replay().mean.clone() if mode == "regression" else graphed.replay().probs.clone()
    post.sample_bank(5, bank, sample_offset=50)
    got, rep = bank.predictive(x, sigma=0.7, **kw), graphed.replay()
    for f in got._fields:
        a = getattr(got, f)
        assert (a is None and getattr(rep, f) is None) or torch.equal(a, getattr(rep, f)), f
    now = rep.mean if mode == "regression" else rep.probs
    assert not torch.equal(now, first_mean) and bool(torch.isfinite(now).all())
    sc = bank.score(x, y, sigma=0.7)
    assert sc.read().n == 5
    if mode == "classification":
        preds, probs = bank.predict_mc(x)
        assert preds.shape == (5,) and torch.allclose(probs.sum(1), torch.ones(5, device=dev), atol=1e-5)

    # SWAG-Diagonal as a BayesianNetwork: mu the mean's bits, rho from fp64
    bn = post.network(scale=0.5)
    mus = [t for l in (bn.l1, bn.l2, bn.l3) for t in (l.weight_mu, l.bias_mu)]
    rhos = [t for l in (bn.l1, bn.l2, bn.l3) for t in (l.weight_rho, l.bias_rho)]
    for mu, rho, a, v in zip(mus, rhos, post.mean_views(), post._views(post.m2)):
        assert torch.equal(mu.data.view(a.shape), a)
        sig = torch.sqrt(0.5 * torch.clamp(v.double() / 4, min=1e-30))
        assert torch.allclose(torch.nn.functional.softplus(rho.data.double()).view(a.shape), sig, rtol=1e-5, atol=0)
    if mode == "classification":
        preds, probs = bn.predict_mc(x, 4)
        assert preds.shape == (5,) and bool(torch.isfinite(probs).all())

    # swa() copies the mean's bits
    other = _mlp(dev, mode, dropout, seed=9)
    assert post.swa(into=other) is other
    assert all(torch.equal(p.detach(), a) for p, a in zip(other.parameters(), post.mean_views()))

    # the posterior's state dict round-trips in place
    post2 = swag.SwagPosterior(other, rank=3)
    held = (post2.mean.data_ptr(), post2.m2.data_ptr(), post2.dev.data_ptr(), post2.count_word.data_ptr())
    post2.load_state_dict(post.state_dict())
    assert held == (post2.mean.data_ptr(), post2.m2.data_ptr(), post2.dev.data_ptr(), post2.count_word.data_ptr())
    assert torch.equal(post2.mean, post.mean) and torch.equal(post2.dev, post.dev) and post2.count() == 4
    assert sgmcmc._read_word(post2.step_word) == 13


def test_momentum_run_and_state_dicts(dev):
    """momentum 0.9: graph replays equal eager launches; the state dict carries torch.optim.SGD's keys and loads into it (and
    back) with the momentum tensors a captured step holds left in place."""
    X, Y = _data(dev, "classification")
    base = _mlp(dev, "classification")
    out = {}
    for how in ("graph", "eager"):
        bnn_hip.manual_seed(2026)
        net = copy.deepcopy(base)
        opt, post = net.swag(LR, momentum=0.9, weight_decay=WD, start=4, every=2, rank=3)
        before = _state(net, opt, post)
        assert len(before[1]) == 6 and all(not m.any() for m in before[1])
        step = net.graphed_train_step(opt, X[:5], Y[:5], capture=how == "graph")
        assert _equal(_state(net, opt, post), before)
        for j in range(12):
            step.step(X[5 * j:5 * j + 5], Y[5 * j:5 * j + 5])
        out[how] = (net, opt, post, _state(net, opt, post), step)
    net, opt, post, snap, step = out["graph"]
    assert _equal(snap, out["eager"][3]) and post.count() == 4 and all(m.any() for m in snap[1])
    # a constant SWA rate switched in on the host reaches the captured step through the device word
    opt.param_groups[0]["lr"] = 0.005
    step.step(X[:5], Y[:5])
    assert float(opt._dev[0][0]) == float(np.float32(0.005))
    # into torch.optim.SGD and back
    sd = opt.state_dict()
    assert all(s["step"] == 13 for s in sd["state"].values()) and sd["param_groups"][0]["momentum"] == 0.9
    tnet = copy.deepcopy(net)
    topt = torch.optim.SGD(tnet.parameters(), lr=1.0)
    topt.load_state_dict(sd)
    assert topt.param_groups[0]["lr"] == 0.005 and topt.param_groups[0]["weight_decay"] == WD
    assert all(torch.equal(topt.state[q]["momentum_buffer"], opt.state[p]["momentum_buffer"])
               for p, q in zip(net.parameters(), tnet.parameters()))
    held = [opt.state[p]["momentum_buffer"].data_ptr() for p in net.parameters()] + [opt._dev[0][0].data_ptr()]
    was = [opt.state[p]["momentum_buffer"].clone() for p in net.parameters()]
    tsd = copy.deepcopy(topt.state_dict())
    for s in tsd["state"].values():
        s["momentum_buffer"] = s["momentum_buffer"] * 2
    opt.load_state_dict(tsd)
    assert held == [opt.state[p]["momentum_buffer"].data_ptr() for p in net.parameters()] + [opt._dev[0][0].data_ptr()]
    assert all(torch.equal(opt.state[p]["momentum_buffer"], 2 * m) for p, m in zip(net.parameters(), was))
    assert opt.device_step() == 13 and opt.param_groups[0]["capturable"] is True
    step.step(X[:5], Y[:5])                                           # the captured step still runs on the loaded state
    assert opt.device_step() == 14


# ---------------------------------------------------------------------------------------------- 9. refusals
def test_refusals(dev):
    import networks
    from bnn_hip.ensemble import EnsembleTrainStep
    X, Y = _data(dev, "classification")
    net = _mlp(dev, "classification")
    opt, post = net.swag(0.1, rank=3)
    with pytest.raises(BnnHipError, match="at least 2"):
        post.sample_bank(3)
    with pytest.raises(BnnHipError, match="at least 2"):
        post.network()
    with pytest.raises(BnnHipError, match="nothing has been collected"):
        post.swa()
    _, post0 = net.swag(0.1, rank=0)
    assert post0.dev is None
    sgmcmc._set_word(post0.count_word, 3)
    with pytest.raises(BnnHipError, match="low_rank=False"):
        post0.sample_bank(3)
    assert post0.sample_bank(3, low_rank=False, sample_offset=0).count() == 3
    other = _mlp(dev, "regression")
    with pytest.raises(BnnHipError, match="other parameter shapes"):
        swag.FusedSWAG(net.parameters(), 0.1, swag=swag.SwagPosterior(other))
    sgmcmc._set_word(post.count_word, 3)
    with pytest.raises(BnnHipError, match="parameter shapes"):
        post.sample_bank(3, other.weight_bank(3))
    with pytest.raises(BnnHipError, match="parameter shapes"):
        post.swa(into=other)
    with pytest.raises(BnnHipError, match="ROCm device"):
        networks.MLP(dict(input_shape=16, classes=3, batch_size=5, hidden_units=8, mode="classification")).swag(0.1)
    opt_nc, _ = net.swag(0.1, capturable=False)
    with pytest.raises(BnnHipError, match="capturable"):
        net.graphed_train_step(opt_nc, X[:5], Y[:5])
    ps = list(net.parameters())
    with pytest.raises(BnnHipError, match="one group"):
        swag.FusedSWAG([dict(params=ps[:2]), dict(params=ps[2:])], 0.1, swag=post)
    with pytest.raises(BnnHipError, match="rank"):
        net.swag(0.1, rank=L.SWAG_MAX_RANK + 1)
    for bad in (dict(nesterov=True, momentum=0.9), dict(dampening=0.1), dict(maximize=True)):
        with pytest.raises(BnnHipError, match="not supported"):
            net.swag(0.1, **bad)
    sd = torch.optim.SGD(net.parameters(), lr=0.1, momentum=0.9, nesterov=True).state_dict()
    with pytest.raises(BnnHipError, match="not supported"):
        opt.load_state_dict(sd)
    with pytest.raises(BnnHipError):                                 # MultiSWAG is not built: the ensemble step keeps refusing
        EnsembleTrainStep(net.ensemble(2, seeds=range(2)), opt, X[:5], Y[:5])
    # an eager step without a gradient on every parameter
    for p in ps:
        p.grad = None
    with pytest.raises(BnnHipError, match="gradient"):
        opt.step()
