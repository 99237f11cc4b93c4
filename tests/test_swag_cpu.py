"""CPU-side checks of SWAG (bnn_swag_step, bnn_swag_sample, bnn_hip.swag; include/bnn_hip.h F22; no GPU): the entry points exist
and the ABI version is unchanged, the ctypes mirrors match the header, malformed arguments are refused on the host in the
documented order, the host's collect predicate and coefficient table agree with the fp64 formulas, SWAG-Diagonal's rho agrees
with fp64, and the numpy restatement (tests/swag_ref.py) is checked on its own: the two streams against the oracle's generator,
Welford against the fp64 moments, the chain's start / every / ring, and the draw's covariance against the paper's."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import swag_ref as R
from test_bandit_cpu import _layout
from test_laplace_cpu import ABI, ALIGN, ENUM, FAKE, NULL, SHAPE, _args, _merge, _refused

NEW = ("bnn_swag_step", "bnn_swag_sample")
SEED = 0x5EED0123456789AB


def _L():
    from bnn_hip import _lib as L
    return L


def test_swag_exports_and_abi_version():
    L = _L()
    lib = L.load()
    assert lib.bnn_version() == 9 == L.ABI_VERSION
    for name in NEW:
        assert name in L.EXPORTS and hasattr(lib, name)
    import bnn_hip
    import networks
    from bnn_hip import ops, swag
    assert bnn_hip.FusedSWAG is swag.FusedSWAG and bnn_hip.SwagPosterior is swag.SwagPosterior
    assert "FusedSWAG" in bnn_hip.__all__ and "SwagPosterior" in bnn_hip.__all__
    for name in ("swag_step", "swag_sample", "swag_collects", "swag_coefficients"):
        assert callable(getattr(ops, name))
    for name in ("count", "variance", "swa", "state_dict", "load_state_dict", "sample_bank", "network"):
        assert callable(getattr(swag.SwagPosterior, name))
    assert callable(networks.MLP.swag) and callable(networks.MLP_Dropout.swag)
    header = open(_layout.__globals__["HEADER"]).read()
    for name in NEW:
        assert f"int {name}(const {name}_args* args, void* stream);" in header
    assert "F22" in header and "#define BNN_HIP_ABI_VERSION 9" in header and "#define BNN_EPS_MAP_VERSION 2" in header
    assert "#define BNN_SWAG_MAX_RANK 32" in header and "#define BNN_SWAG_MAX_MEMBERS 64" in header


def test_swag_struct_layouts_match_the_header(tmp_path):
    L = _L()
    _layout(tmp_path, L.SwagStepArgs, "bnn_swag_step_args",
            [("BNN_SWAG_MAX_RANK", L.SWAG_MAX_RANK), ("BNN_SWAG_MAX_MEMBERS", L.SWAG_MAX_MEMBERS),
             ("BNN_SGMCMC_MAX_TENSORS", L.SGMCMC_MAX_TENSORS), ("BNN_HIP_ABI_VERSION", L.ABI_VERSION)])
    _layout(tmp_path, L.SwagSampleArgs, "bnn_swag_sample_args")
    assert L.SWAG_MAX_RANK == R.MAX_RANK and L.SWAG_MAX_MEMBERS == R.MAX_MEMBERS and L.SGMCMC_MAX_TENSORS == R.MAX_TENSORS
    assert L.SWAG_NOISE_WORD3 == R.WORD3 == 5 and L.KFAC_NOISE_WORD3 == 4


# ---------------------------------------------------------------------------------------------- the documented error order
def _step(**over):
    L = _L()
    two = {0: FAKE, 1: FAKE}
    d = dict(n_tensors=2, param=two, grad=two, momentum=two, numel={0: 5000, 1: 7}, lr=0.1, momentum_factor=0.9, weight_decay=1e-4,
             start=4, every=2, rank=3)
    return _args(L.SwagStepArgs, ("lr_device", "mean", "m2", "dev", "step", "count", "ticket"), **_merge(d, over))


def _sample(**over):
    L = _L()
    d = dict(n_tensors=2, numel={0: 5000, 1: 7}, rank=3, members=4, first=1, capacity=5, low_rank=1, eps_mode=L.EPS_MEMORY, c_d=0.7,
             var_clamp=1e-30, sample_base=9, seed=7)
    return _args(L.SwagSampleArgs, ("mean", "m2", "dev", "count", "z1", "z2", "bank"), **_merge(d, over))


def test_swag_step_argument_errors():
    L = _L()
    fn = L.load().bnn_swag_step
    nan = float("nan")
    _refused(fn, _step, C.sizeof(L.SwagStepArgs), [
        (SHAPE, (dict(n_tensors=0), dict(n_tensors=-1), dict(n_tensors=L.SGMCMC_MAX_TENSORS + 1), dict(rank=-1),
                 dict(rank=L.SWAG_MAX_RANK + 1), dict(every=0), dict(lr=-0.1), dict(lr=nan), dict(momentum_factor=-0.5),
                 dict(weight_decay=nan), dict(numel={1: 0}), dict(numel={0: -5}), dict(numel={0: (1 << 34) + 1}))),
        (NULL, (dict(step=None), dict(count=None), dict(ticket=None), dict(mean=None), dict(m2=None), dict(dev=None),
                dict(param={1: None}), dict(grad={0: None}), dict(momentum={1: None}), dict(momentum={0: None}))),
        (ALIGN, (dict(param={0: FAKE + 4}), dict(grad={1: FAKE + 8}), dict(momentum={0: FAKE + 4, 1: FAKE + 4}),
                 dict(mean=FAKE + 4), dict(m2=FAKE + 8), dict(dev=FAKE + 4), dict(lr_device=FAKE + 2), dict(step=FAKE + 2),
                 dict(count=FAKE + 1), dict(ticket=FAKE + 2))),
    ])
    # what a mode does not need may be NULL: rank 0 reads no dev; no momentum at all; no device rate
    assert fn(C.byref(_step(rank=0, dev=None, param={0: None})), None) == NULL
    assert fn(C.byref(_step(rank=0, dev=FAKE + 4, step=FAKE + 2)), None) == ALIGN              # (an unread dev is not checked)
    assert fn(C.byref(_step(momentum={0: None, 1: None}, lr_device=None, step=FAKE + 2)), None) == ALIGN
    # shape before NULL, NULL before alignment
    assert fn(C.byref(_step(every=0, mean=None, step=FAKE + 2)), None) == SHAPE
    assert fn(C.byref(_step(mean=None, step=FAKE + 2)), None) == NULL


def test_swag_sample_argument_errors():
    L = _L()
    fn = L.load().bnn_swag_sample
    _refused(fn, _sample, C.sizeof(L.SwagSampleArgs), [
        (SHAPE, (dict(n_tensors=0), dict(n_tensors=L.SGMCMC_MAX_TENSORS + 1), dict(rank=-1), dict(rank=L.SWAG_MAX_RANK + 1),
                 dict(members=0), dict(members=L.SWAG_MAX_MEMBERS + 1, capacity=200), dict(first=-1), dict(capacity=0),
                 dict(first=2), dict(rank=0), dict(var_clamp=-1.0), dict(var_clamp=float("nan")), dict(numel={1: 0}),
                 dict(numel={0: (1 << 34) + 1}))),
        (ENUM, (dict(eps_mode=3), dict(eps_mode=-1))),
        (NULL, (dict(mean=None), dict(m2=None), dict(count=None), dict(bank=None), dict(dev=None), dict(z1=None), dict(z2=None))),
        (ALIGN, (dict(mean=FAKE + 4), dict(m2=FAKE + 8), dict(dev=FAKE + 4), dict(bank=FAKE + 8), dict(z1=FAKE + 4),
                 dict(z2=FAKE + 2), dict(count=FAKE + 1))),
    ])
    # SWAG-Diagonal reads no dev and no z2, rank 0 allowed; the on-chip streams and BNN_EPS_ZERO read no z1 / z2
    assert fn(C.byref(_sample(low_rank=0, rank=0, dev=None, z2=None, count=FAKE + 1)), None) == ALIGN
    assert fn(C.byref(_sample(low_rank=0, dev=FAKE + 4, z2=FAKE + 2, count=FAKE + 1)), None) == ALIGN
    for mode in (L.EPS_PHILOX, L.EPS_ZERO):
        assert fn(C.byref(_sample(eps_mode=mode, z1=None, z2=None, count=FAKE + 1)), None) == ALIGN
    assert fn(C.byref(_sample(members=L.SWAG_MAX_MEMBERS, first=0, capacity=L.SWAG_MAX_MEMBERS, count=FAKE + 1)), None) == ALIGN
    # shape before enum, enum before NULL, NULL before alignment
    assert fn(C.byref(_sample(members=0, eps_mode=9, mean=None)), None) == SHAPE
    assert fn(C.byref(_sample(eps_mode=9, mean=None, count=FAKE + 1)), None) == ENUM
    assert fn(C.byref(_sample(mean=None, count=FAKE + 1)), None) == NULL


# ---------------------------------------------------------------------------------------------- host logic
def test_collect_predicate_and_coefficients():
    from bnn_hip import ops
    for start, every in ((0, 1), (4, 2), (3, 5), (7, 1)):
        for k in range(40):
            want = k >= start and (k - start + 1) % every == 0
            assert ops.swag_collects(k, start, every) == want == R.collects(k, start, every)
    assert [k for k in range(12) if ops.swag_collects(k, 4, 2)] == [5, 7, 9, 11]               # the end of every 2-step "epoch"
    assert ops.swag_collects(2 ** 32 + 5, 4, 2) and not ops.swag_collects(2 ** 32 + 4, 4, 2)  # the word is 32 bits
    for scale in (1.0, 0.5, 3.7):
        c_d, c_lr = ops.swag_coefficients(scale, True)
        assert c_d == float(np.float32(math.sqrt(scale / 2))) and c_lr.dtype == np.float32 and c_lr.shape == (33,)
        assert c_lr[0] == 0 and c_lr[1] == 0
        for e in range(2, 33):
            assert float(c_lr[e]) == float(np.float32(math.sqrt(scale / (2 * (e - 1)))))
        rd, rl = R.coefficients(scale, True)
        assert float(rd) == c_d and np.array_equal(rl, c_lr)
        c_d, c_lr = ops.swag_coefficients(scale, False)
        assert c_d == float(np.float32(math.sqrt(scale))) and not c_lr.any()
        rd, rl = R.coefficients(scale, False)
        assert float(rd) == c_d and np.array_equal(rl, c_lr)
    with pytest.raises(ops.BnnHipError):
        ops.swag_coefficients(-1.0)
    offs, stride = R.layout([1, 5, 37, 1201, 4096, 4100])
    assert ops.bank_layout([1, 5, 37, 1201, 4096, 4100]) == (tuple(offs), stride) and stride == 64 * 3 + 1216 + 4096 + 4160


def test_host_side_refusals():
    import networks
    from bnn_hip import ops, swag
    from bnn_hip.ops import BnnHipError
    mp = dict(input_shape=5, classes=3, batch_size=4, hidden_units=6, mode="classification")
    with pytest.raises(BnnHipError, match="ROCm device"):                       # CPU parameters: no fallback
        networks.MLP(mp).swag(0.1)
    with pytest.raises(BnnHipError, match="rank"):
        swag.SwagPosterior(networks.MLP(mp), rank=33)
    z = torch.zeros(64)
    w = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(BnnHipError):
        ops.swag_step([torch.zeros(4)], [torch.zeros(4)], lr=0.1, mean=z, m2=z, dev=None, step=w, count=w,
                      ticket=torch.zeros(16, dtype=torch.int32))
    with pytest.raises(BnnHipError):
        ops.swag_sample([4], z, z, None, w, torch.zeros(2, 64), members=2, low_rank=False)
    with pytest.raises(BnnHipError, match="low_rank=False"):
        ops.swag_sample([4], z, z, None, w, torch.zeros(2, 64), members=2)
    with pytest.raises(BnnHipError):
        ops.swag_sample([4], z, z, torch.zeros(33, 64), w, torch.zeros(2, 64), members=2)
    with pytest.raises(BnnHipError):
        ops.swag_sample([4], z, z, None, w, torch.zeros(2, 64), members=65, low_rank=False)
    for bad in (dict(nesterov=True), dict(dampening=0.1), dict(maximize=True)):
        with pytest.raises(BnnHipError, match="not supported"):
            swag._swag_supported(bad)
    swag._swag_supported(dict(momentum=0.9, weight_decay=1e-4, dampening=0, nesterov=False, maximize=False))


def test_diag_rho_against_fp64():
    """rho = softplus^-1(sqrt(scale max(m2 / n, clamp))): softplus(rho) gives sigma back to fp32 rounding over 30 decades."""
    from bnn_hip import swag
    rng = np.random.default_rng(5)
    m2 = (10.0 ** rng.uniform(-20, 6, 4000)).astype(np.float32)
    m2[:3] = [0.0, 1e-38, 1e30]
    n, scale, clamp = 7, 0.5, 1e-30
    rho = swag.diag_rho(torch.from_numpy(m2), n, scale, clamp)
    assert rho.dtype == torch.float32 and rho.shape == (4000,) and bool(torch.isfinite(rho).all())
    sigma = np.sqrt(scale * np.maximum(m2.astype(np.float64) / n, clamp))
    want = np.where(sigma > 30, sigma, np.log(np.expm1(np.minimum(sigma, 30.0))))
    np.testing.assert_allclose(rho.numpy().astype(np.float64), want, rtol=2.0 ** -23, atol=1e-12)
    # rho's fp32 rounding (|rho| 2^-24) moves sigma by at most that (d sigma / d rho = sigmoid <= sigma / ... <= 1 relative to
    # sigma when rho << 0): |rho| <= 35 at the clamp, so 40 * 2^-24 relative
    r64 = rho.numpy().astype(np.float64)
    back = np.where(r64 > 40, r64, np.log1p(np.exp(np.minimum(r64, 40.0))))     # (softplus(rho) = rho to fp64 beyond 40)
    np.testing.assert_allclose(back, sigma, rtol=40 * 2.0 ** -24)


# ---------------------------------------------------------------------------------------------- the restatement itself
def test_restated_streams_are_the_oracle_generator_on_word_5():
    from oracle import bnn_oracle as O
    import sgmcmc_ref
    e = R.z1(SEED, 7, 3, 1201)
    assert e.shape == (1201,) and e.dtype == np.float32 and np.isfinite(e).all()
    r = O.philox4x32(np.uint32(275), np.uint32(7), np.uint32(3), np.uint32(5), SEED & 0xFFFFFFFF, SEED >> 32)
    assert O.box_muller(r[2], r[3])[0] == e[1102] and O.box_muller(r[0], r[1])[1] == e[1101]
    z = R.z2(SEED, 7, 32)
    r = O.philox4x32(np.uint32(5), np.uint32(7), np.uint32(16), np.uint32(5), SEED & 0xFFFFFFFF, SEED >> 32)
    assert O.box_muller(r[2], r[3])[1] == z[23] and np.array_equal(R.z2(SEED, 7, 3), z[:3])
    assert np.array_equal(R.z1(SEED, 7, 3, 37), e[:37])
    # draws, tensors, the z2 stream, F19's word 3 = 3 and the epsilon map's word 3 = 0 are other streams
    for other in (R.z1(SEED, 8, 3, 1201), R.z1(SEED, 7, 4, 1201), R.z1(SEED + 1, 7, 3, 1201), R.z1(SEED, 7, 16, 1201),
                  sgmcmc_ref.noise(SEED, 3, 7, 1201), O.philox_normal(SEED, 3, 7, 1, 1201)[0]):
        assert not np.array_equal(other, e) and abs(np.corrcoef(other, e)[0, 1]) < 0.15
    assert np.array_equal(R.z1(SEED, 16, R.Z2_STREAM, 32), R.z2(SEED, 16, 32))
    big = R.z1(SEED, 0, 15, 1 << 16)
    assert abs(big.mean()) < 4 / 256 and abs(big.var() - 1) < 0.03


def test_restated_step_is_sgd_with_momentum_in_fp32():
    rng = np.random.default_rng(1)
    p, g = rng.standard_normal(500).astype(np.float32), rng.standard_normal(500).astype(np.float32)
    v = np.zeros(500, np.float32)
    lr, mu, wd = 0.05, 0.9, 1e-3
    p64, v64 = p.astype(np.float64), v.astype(np.float64)
    for _ in range(3):
        p, v = R.sgd_update(p, v, g, lr, mu, wd)
        gg = g + wd * p64
        v64 = mu * v64 + gg
        p64 = p64 - lr * v64
    np.testing.assert_allclose(p, p64, rtol=0, atol=2e-6)
    np.testing.assert_allclose(v, v64, rtol=0, atol=4e-6)
    q, none = R.sgd_update(p, None, g, lr, 0.0, 0.0)
    assert none is None and np.array_equal(q, R.fma32(np.float32(-lr), g, p))


def test_restated_welford_chain_and_ring():
    """start 4, every 2, rank 3, 12 steps: steps 5, 7, 9, 11 collect; the ring holds deviations 3, 1, 2 (row n % 3); the moments
    equal the fp64 mean and population variance of the four iterates; the padding is never written."""
    rng = np.random.default_rng(2)
    params = [(1 + 1e-3 * rng.standard_normal(n)).astype(np.float32) for n in (3, 65)]
    stride = R.layout([3, 65])[1]
    mean, m2 = np.full(stride, 7.0, np.float32), np.full(stride, 7.0, np.float32)
    dev = np.full((3, stride), 7.0, np.float32)
    for o, n in ((0, 3), (64, 65)):
        mean[o:o + n] = 0
        m2[o:o + n] = 0
    ch = R.Chain(params, lr=0.1, mu=0.9, momentum=True, start=4, every=2, rank=3, mean=mean, m2=m2, dev=dev)
    its = []
    for k in range(12):
        ch.step([(1e-2 * rng.standard_normal(t.shape)).astype(np.float32) for t in ch.p])
        if R.collects(k, 4, 2):
            its.append([t.copy() for t in ch.p])
    assert ch.k == 12 and ch.n == 4 and ch.collected_at == [5, 7, 9, 11]
    for t, (o, n) in enumerate(((0, 3), (64, 65))):
        X = np.stack([it[t] for it in its]).astype(np.float64)
        np.testing.assert_allclose(mean[o:o + n], X.mean(0), rtol=3e-7)
        np.testing.assert_allclose(m2[o:o + n] / 4, X.var(0), rtol=1e-3)          # (spread 1e-2 around 1: d carries ~1e-5 relative)
        # row 0 was overwritten by iterate 3 (n = 3 -> 3 % 3 = 0): deviation from the mean of all four
        np.testing.assert_allclose(dev[0, o:o + n], X[3] - X.mean(0), atol=2e-7)
        np.testing.assert_allclose(dev[1, o:o + n], X[1] - X[:2].mean(0), atol=2e-7)
        np.testing.assert_allclose(dev[2, o:o + n], X[2] - X[:3].mean(0), atol=2e-7)
    for buf in (mean, m2, dev[0], dev[1], dev[2]):
        assert (buf[3:64] == 7.0).all() and (buf[129:] == 7.0).all()
    # rank 0 keeps no ring; the first collected iterate is the mean and leaves m2 at 0
    c0 = R.Chain(params, lr=0.1, start=0, every=1, rank=0)
    c0.step([np.zeros_like(t) for t in params])
    assert c0.dev is None and c0.n == 1 and np.array_equal(c0.mean[:3], params[0]) and not c0.m2.any()


def test_restated_draw_has_the_paper_covariance():
    """The draw is linear in (z1, z2): pushing unit vectors through R.draw gives its matrix A, and A A^T is R.covariance; with
    unrounded coefficients that is the paper's scale (diag(var) / 2 + D^T D / (2 (Keff - 1)))."""
    rng = np.random.default_rng(3)
    P, K, n = 11, 3, 5
    mean = rng.standard_normal(P).astype(np.float32)
    m2 = (rng.uniform(0.5, 2.0, P) * n).astype(np.float32)
    dev = (0.3 * rng.standard_normal((K, P))).astype(np.float32)
    zero1, zero2 = np.zeros(P, np.float32), np.zeros(K, np.float32)
    assert np.array_equal(R.draw(mean, m2, dev, n, zero1, zero2), mean)
    cols = []
    for i in range(P):
        e = zero1.copy()
        e[i] = 1
        cols.append(R.draw(zero1, m2, dev, n, e, zero2, scale=0.7).astype(np.float64))
    for j in range(K):
        e = zero2.copy()
        e[j] = 1
        cols.append(R.draw(zero1, m2, dev, n, zero1, e, scale=0.7).astype(np.float64))
    A = np.stack(cols, axis=1)
    S = R.covariance(m2, dev, n, scale=0.7)
    np.testing.assert_allclose(A @ A.T, S, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(S, R.swag_covariance(m2.astype(np.float64) / n, dev, K, 0.7), rtol=1e-6, atol=1e-9)
    # n < rank: only the rows collected so far enter, with the factor of Keff = n
    S2 = R.covariance(m2, dev, 2, scale=1.0)
    np.testing.assert_allclose(S2, R.swag_covariance(m2.astype(np.float64) / 2, dev, 2, 1.0), rtol=1e-6, atol=1e-9)
    Sd = R.covariance(m2, dev, n, scale=0.7, low_rank=False)
    np.testing.assert_allclose(Sd, 0.7 * np.diag(m2.astype(np.float64) / n), rtol=1e-6)
