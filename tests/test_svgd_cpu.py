"""CPU-side checks of SVGD / kde-WGD (bnn_svgd_dist, bnn_svgd_coef, bnn_svgd_direction, bnn_hip.svgd; include/bnn_hip.h F23; no
GPU): the entry points exist and the ABI version is unchanged, the ctypes mirrors match the header, malformed arguments are
refused on the host in the documented order, the host-side refusals have their sentences, and the fp64 restatement
(tests/svgd_ref.py) is tied to the DEFINITION of the two updates -- phi with the kernel's gradient taken by torch autograd --
and moves particles onto a 2-D Gaussian."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import svgd_ref as R
from test_bandit_cpu import _layout
from test_laplace_cpu import ABI, ALIGN, ENUM, FAKE, NULL, SHAPE, _args, _refused

NEW = ("bnn_svgd_dist", "bnn_svgd_coef", "bnn_svgd_direction")
HELPERS = ("bnn_svgd_chunks",)


def _L():
    from bnn_hip import _lib as L
    return L


def test_svgd_exports_and_abi_version():
    L = _L()
    lib = L.load()
    assert lib.bnn_version() == 9 == L.ABI_VERSION
    for name in NEW + HELPERS:
        assert name in L.EXPORTS and hasattr(lib, name)
    import bnn_hip
    from bnn_hip import ensemble, ops, svgd
    assert bnn_hip.SteinTransform is svgd.SteinTransform and "SteinTransform" in bnn_hip.__all__
    assert "`svgd`" in bnn_hip.__doc__
    for name in ("svgd_dist", "svgd_coef", "svgd_direction", "svgd_chunks"):
        assert callable(getattr(ops, name))
    assert callable(ensemble.DeepEnsemble.svgd) and callable(svgd.SteinTransform.enqueue) and callable(svgd.SteinTransform.read)
    import inspect
    assert "transform" in inspect.signature(ensemble.EnsembleTrainStep.__init__).parameters
    assert "transform" in inspect.signature(ensemble.DeepEnsemble.graphed_train_step).parameters
    sig = inspect.signature(svgd.SteinTransform.__init__).parameters
    assert list(sig)[1:] == ["ens", "dataset_size", "batch_size", "prior_precision", "temperature", "method", "bandwidth"]
    assert sig["prior_precision"].default == 1.0 and sig["temperature"].default == 1.0 and sig["method"].default == "svgd"
    assert sig["bandwidth"].default is None
    header = open(_layout.__globals__["HEADER"]).read()
    for name in NEW:
        assert f"int {name}(const {name}_args* args, void* stream);" in header
    assert "int32_t bnn_svgd_chunks(int64_t stride);" in header
    assert "F23" in header and "#define BNN_HIP_ABI_VERSION 9" in header and "#define BNN_EPS_MAP_VERSION 2" in header
    assert "#define BNN_SVGD_MAX_MEMBERS 64" in header and f"#define BNN_SVGD_CHAIN {R.CHAIN}" in header


def test_svgd_struct_layouts_match_the_header(tmp_path):
    L = _L()
    _layout(tmp_path, L.SvgdDistArgs, "bnn_svgd_dist_args",
            [("BNN_SVGD_MAX_MEMBERS", L.SVGD_MAX_MEMBERS), ("BNN_SVGD_CHUNK", L.SVGD_CHUNK), ("BNN_SVGD_CHAIN", L.SVGD_CHAIN),
             ("BNN_SVGD_SVGD", L.SVGD_SVGD), ("BNN_SVGD_WGD", L.SVGD_WGD), ("BNN_SVGD_RECORD_DOUBLES(7)", L.svgd_record_doubles(7)),
             ("BNN_HIP_ABI_VERSION", L.ABI_VERSION)])
    _layout(tmp_path, L.SvgdCoefArgs, "bnn_svgd_coef_args")
    _layout(tmp_path, L.SvgdDirectionArgs, "bnn_svgd_direction_args")
    assert (L.SVGD_MAX_MEMBERS, L.SVGD_CHUNK, L.SVGD_CHAIN) == (R.MAX_MEMBERS, R.CHUNK, R.CHAIN)
    assert L.svgd_record_doubles(64) == 64 * 64 + 64 + 2 and L.svgd_record_doubles(1) == 4


# ---------------------------------------------------------------------------------------------- the documented error order
def _dist(**over):
    return _args(_L().SvgdDistArgs, ("bank", "partials"), **dict(dict(members=9, stride=6400), **over))


def _coef(**over):
    d = dict(members=9, chunks=2, method=0, grad_scale=10.0, tau=1.0, bandwidth=0.0)
    return _args(_L().SvgdCoefArgs, ("partials", "coef", "record"), **dict(d, **over))


def _direction(**over):
    return _args(_L().SvgdDirectionArgs, ("coef", "bank", "bucket"), **dict(dict(members=9, stride=6400), **over))


def test_svgd_dist_argument_errors():
    L = _L()
    fn = L.load().bnn_svgd_dist
    _refused(fn, _dist, C.sizeof(L.SvgdDistArgs), [
        (SHAPE, (dict(members=0), dict(members=-1), dict(members=L.SVGD_MAX_MEMBERS + 1), dict(stride=0), dict(stride=63),
                 dict(stride=100), dict(stride=-64), dict(stride=(1 << 34) + 64))),
        (NULL, (dict(bank=None), dict(partials=None))),
        (ALIGN, (dict(bank=FAKE + 4), dict(bank=FAKE + 8), dict(partials=FAKE + 2))),
    ])
    assert fn(C.byref(_dist(members=0, bank=None)), None) == SHAPE               # shape before NULL, NULL before alignment
    assert fn(C.byref(_dist(bank=None, partials=FAKE + 2)), None) == NULL
    assert fn(C.byref(_dist(members=L.SVGD_MAX_MEMBERS, stride=64, partials=FAKE + 2)), None) == ALIGN   # (the limits are legal)
    assert fn(C.byref(_dist(members=1, stride=1 << 34, partials=FAKE + 2)), None) == ALIGN


def test_svgd_coef_argument_errors():
    L = _L()
    fn = L.load().bnn_svgd_coef
    nan, inf = float("nan"), float("inf")
    _refused(fn, _coef, C.sizeof(L.SvgdCoefArgs), [
        (SHAPE, (dict(members=0), dict(members=L.SVGD_MAX_MEMBERS + 1), dict(chunks=0), dict(chunks=(1 << 22) + 1),
                 dict(grad_scale=0.0), dict(grad_scale=-1.0), dict(grad_scale=nan), dict(grad_scale=inf), dict(tau=-1.0),
                 dict(tau=nan), dict(tau=inf), dict(bandwidth=-0.5), dict(bandwidth=nan), dict(bandwidth=inf))),
        (ENUM, (dict(method=2), dict(method=-1))),
        (NULL, (dict(partials=None), dict(coef=None), dict(record=None))),
        (ALIGN, (dict(partials=FAKE + 2), dict(coef=FAKE + 1), dict(record=FAKE + 4))),
    ])
    assert fn(C.byref(_coef(chunks=0, method=5, coef=None)), None) == SHAPE      # shape, enum, NULL, alignment
    assert fn(C.byref(_coef(method=5, coef=None, record=FAKE + 4)), None) == ENUM
    assert fn(C.byref(_coef(coef=None, record=FAKE + 4)), None) == NULL
    for ok in (dict(method=1), dict(tau=0.0), dict(bandwidth=2.5), dict(members=1), dict(members=L.SVGD_MAX_MEMBERS, chunks=1 << 22)):
        assert fn(C.byref(_coef(record=FAKE + 4, **ok)), None) == ALIGN, ok


def test_svgd_direction_argument_errors():
    L = _L()
    fn = L.load().bnn_svgd_direction
    _refused(fn, _direction, C.sizeof(L.SvgdDirectionArgs), [
        (SHAPE, (dict(members=0), dict(members=L.SVGD_MAX_MEMBERS + 1), dict(stride=0), dict(stride=6401), dict(stride=32),
                 dict(stride=(1 << 34) + 64))),
        (NULL, (dict(coef=None), dict(bank=None), dict(bucket=None))),
        (ALIGN, (dict(coef=FAKE + 2), dict(bank=FAKE + 4), dict(bucket=FAKE + 8))),
    ])
    assert fn(C.byref(_direction(stride=32, bank=None)), None) == SHAPE
    assert fn(C.byref(_direction(bank=None, bucket=FAKE + 8)), None) == NULL


def test_host_side_refusals():
    """No device: every refusal of SteinTransform and of the ops has its sentence, CPU tensors included."""
    import types
    import networks
    from bnn_hip import ops
    from bnn_hip.ensemble import DeepEnsemble
    from bnn_hip.ops import BnnHipError
    from bnn_hip.svgd import SteinTransform
    net = networks.MLP(dict(input_shape=5, classes=3, batch_size=4, hidden_units=6, mode="classification"))
    with pytest.raises(BnnHipError, match="ROCm device only"):                   # a CPU network has no ensemble at all
        net.ensemble(3, seeds=[1, 2, 3])

    class Ens:                                                                   # what SteinTransform reads of an ensemble
        def __init__(self, M):
            self.members, self.bank = M, types.SimpleNamespace(buffer=torch.zeros((M, 128)), stride=128)

        svgd = DeepEnsemble.svgd

    ens = Ens(3)
    kw = dict(dataset_size=100, batch_size=10)
    with pytest.raises(BnnHipError, match="ROCm device only"):                   # CPU tensors: no fallback
        ens.svgd(**kw)
    with pytest.raises(BnnHipError, match="at most 64 members, got 65"):
        SteinTransform(Ens(65), **kw)
    with pytest.raises(BnnHipError, match="method must be one of"):
        ens.svgd(method="stein", **kw)
    with pytest.raises(BnnHipError, match="prior_precision must be >= 0"):
        ens.svgd(prior_precision=-1.0, **kw)
    for t in (0.0, -1.0, float("nan")):
        with pytest.raises(BnnHipError, match="temperature must be > 0"):
            ens.svgd(temperature=t, **kw)
    for h in (0.0, -2.0, float("inf")):
        with pytest.raises(BnnHipError, match="bandwidth must be > 0"):
            ens.svgd(bandwidth=h, **kw)
    with pytest.raises(BnnHipError, match="dataset_size and batch_size"):
        ens.svgd(dataset_size=0, batch_size=10)
    z = torch.zeros((3, 128))
    with pytest.raises(BnnHipError, match="ROCm device only"):
        ops.svgd_dist(z, torch.zeros(3), members=3)
    with pytest.raises(BnnHipError, match="between 1 and 64 members"):
        ops.svgd_dist(z, torch.zeros(3), members=65)
    with pytest.raises(BnnHipError, match="ROCm device only"):
        ops.svgd_direction(torch.zeros((3, 6)), z, z.clone(), members=3)
    with pytest.raises(BnnHipError, match="ROCm device only"):
        ops.svgd_coef(torch.zeros(3), torch.zeros(18), torch.zeros(14, dtype=torch.float64), members=3, chunks=1, grad_scale=1.0, tau=0.0)
    # the chunking: whole tiles, at most 4096 columns, about 512 chunks of a smaller bank
    for stride, want in ((64, 1), (4096, 64), (8256, 129), (32768, 512), (32832, 257), (161856, 506), (2395328, 585), (1 << 34, 1 << 22)):
        assert ops.svgd_chunks(stride) == want == R.chunks(stride), stride
    for bad in (0, 32, 100, -64, (1 << 34) + 64):
        with pytest.raises(BnnHipError, match="multiple of 64"):
            ops.svgd_chunks(bad)


# ---------------------------------------------------------------------------------------------- the restatement itself
def _phi_autograd(theta, g, s, tau, method, h):
    """-d by the DEFINITION, the kernel's gradient from autograd (h a constant of the step).
    svgd: phi_i = (1 / M) sum_j [ k(theta_j, theta_i) (-grad U_j) + grad_{theta_j} k(theta_j, theta_i) ]
    wgd:  v_i   = -grad U_i - sum_j grad_{theta_i} k(theta_i, theta_j) / sum_j k(theta_i, theta_j)"""
    th = torch.from_numpy(theta)
    M = th.shape[0]
    gU = s * torch.from_numpy(g) + tau * th
    k = lambda a, b: torch.exp(-((a - b) ** 2).sum(-1) / h)
    out = []
    for i in range(M):
        if method == "svgd":
            X = th.clone().requires_grad_()
            kv = k(X, th[i])                                                     # k(theta_j, theta_i), j = 0 .. M - 1
            grad = torch.autograd.grad(kv.sum(), X)[0]                           # row j: grad_{theta_j} k(theta_j, theta_i)
            out.append(((kv.detach()[:, None] * -gU) + grad).sum(0) / M)
        else:
            x = th[i].clone().requires_grad_()
            kv = k(x, th)                                                        # k(theta_i, theta_j)
            grad = torch.autograd.grad(kv.sum(), x)[0]
            out.append(-gU[i] - grad / kv.detach().sum())
    return torch.stack(out).numpy()


@pytest.mark.parametrize("method", R.METHODS)
@pytest.mark.parametrize("M", [1, 2, 3, 9])
def test_restated_direction_is_the_definition_with_autograd_kernel_gradients(M, method):
    rng = np.random.default_rng(10 * M + len(method))
    P = 7
    theta, g = rng.standard_normal((M, P)), rng.standard_normal((M, P))
    s, tau = R.energy_scales(600, 32, prior_precision=0.7, temperature=0.5)
    assert s == 600 / 16 and tau == 1.4
    for h in (None, 3.3):
        D2 = R.dist2(theta)
        A, B, med, hh, r = R.coefficients(D2, s, tau, method, h)
        assert med == np.median(D2) and hh == (h if h else (med / math.log(M + 1) if med else 1.0))
        d = A @ g + B @ theta
        np.testing.assert_allclose(-d, _phi_autograd(theta, g, s, tau, method, hh), rtol=1e-10, atol=1e-12)
        np.testing.assert_array_equal(d, R.direction(theta, g, s, tau, method, h))
        assert np.array_equal(D2, D2.T) and not D2.diagonal().any()
        np.testing.assert_allclose(D2, ((theta[:, None] - theta[None]) ** 2).sum(-1), rtol=1e-14)


def test_h_equal_zero_rule_one_member_and_collapsed_members():
    s, tau = 12.5, 0.3
    for method in R.METHODS:
        A, B, med, h, r = R.coefficients(np.zeros((1, 1)), s, tau, method)
        assert med == 0 and h == 1.0 and r[0] == 1.0
        assert A.tolist() == [[s]] and B.tolist() == [[tau]]                     # the plain step, exactly
        theta = np.tile(np.random.default_rng(0).standard_normal(5), (4, 1))    # all members equal: D2 = 0, h = 1, K = 1
        A, B, med, h, r = R.coefficients(R.dist2(theta), s, tau, method)
        assert med == 0 and h == 1.0 and (r == 4).all() and np.isfinite(A).all() and np.isfinite(B).all()
        d = R.direction(theta, np.ones((4, 5)), s, tau, method)
        np.testing.assert_allclose(d, s + tau * theta, rtol=1e-14)               # no repulsion between coincident members
        # more than half of the entries zero (two of three members equal): the median is 0 -> h = 1
        th3 = np.array([[0.0, 0.0], [0.0, 0.0], [3.0, 4.0]])
        med, h = R.bandwidth(R.dist2(th3))
        assert med == 0 and h == 1.0
    assert R.pair_index(0, 1, 5) == 0 and R.pair_index(0, 4, 5) == 3 and R.pair_index(1, 2, 5) == 4 and R.pair_index(3, 4, 5) == 9
    assert sorted(R.pair_index(i, j, 9) for i in range(9) for j in range(i + 1, 9)) == list(range(36))


@pytest.mark.parametrize("method", R.METHODS)
def test_particles_move_onto_a_two_dimensional_gaussian(method):
    """U(theta) = (theta - mu)^T S^-1 (theta - mu) / 2 entered as g = grad U with s = 1, tau' = 0.  40 particles start in a
    tight ball far from mu; after 1500 steps of size 0.05 the particle mean is within 0.1 |mu - start| of mu (it started 1.0
    away in these units) and each marginal variance lies within a factor 2 of the target's (it started a factor 400 below;
    SVGD with the median bandwidth and few particles is known to sit somewhat under it)."""
    rng = np.random.default_rng(7)
    mu = np.array([2.0, -1.0])
    S = np.array([[1.0, 0.6], [0.6, 2.0]])
    Sinv = np.linalg.inv(S)
    start = np.array([-2.0, 2.0])
    theta = start + 0.05 * rng.standard_normal((40, 2))
    v0 = theta.var(axis=0)
    for _ in range(1500):
        theta = theta - 0.05 * R.direction(theta, (theta - mu) @ Sinv, 1.0, 0.0, method)
    assert np.linalg.norm(theta.mean(0) - mu) < 0.1 * np.linalg.norm(start - mu), theta.mean(0)
    ratio = theta.var(axis=0) / np.diag(S)
    assert ((ratio > 0.5) & (ratio < 2.0)).all() and (v0 / np.diag(S) < 0.01).all(), ratio
