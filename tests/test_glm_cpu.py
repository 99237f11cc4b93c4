"""CPU-side checks of the linearised (GLM) predictive of the diagonal Laplace posterior (bnn_laplace_glm_*,
bnn_hip.laplace.DiagLaplace.glm_*; include/bnn_hip.h F18; no GPU): the entry points exist and the ABI version is unchanged, the
ctypes mirrors match the header, malformed arguments are refused on the host with the documented status in the documented order,
the host-side refusals, and the fp64 restatement (tests/glm_ref.py) against an independent form -- J diag(s^2) J^T from autograd
Jacobians -- with the Cholesky, probit and sampler stages checked on their own."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import glm_ref as G
from test_bandit_cpu import _layout
from test_laplace_cpu import ABI, ALIGN, ENUM, FAKE, NULL, SHAPE, _args, _net, _refused

NEW = ("bnn_laplace_glm_layer", "bnn_laplace_glm_finish", "bnn_laplace_glm_sample")


def _L():
    from bnn_hip import _lib as L
    return L


def test_glm_exports_and_abi_version():
    L = _L()
    lib = L.load()
    assert lib.bnn_version() == 9 == L.ABI_VERSION
    for name in NEW:
        assert name in L.EXPORTS and hasattr(lib, name)
    from bnn_hip import laplace, ops
    for name in ("laplace_glm_layer", "laplace_glm_finish", "laplace_glm_sample"):
        assert callable(getattr(ops, name))
    for name in ("glm_moments", "glm_predictive", "glm_predictive_graph", "glm_score"):
        assert callable(getattr(laplace.DiagLaplace, name))
    header = open(_layout.__globals__["HEADER"]).read()
    for name in NEW:
        assert f"int {name}(const {name}_args* args, void* stream);" in header
    assert "F18" in header and "#define BNN_HIP_ABI_VERSION 9" in header and "#define BNN_EPS_MAP_VERSION 2" in header


def test_glm_struct_layouts_match_the_header(tmp_path):
    L = _L()
    _layout(tmp_path, L.LaplaceGlmLayerArgs, "bnn_laplace_glm_layer_args",
            [("BNN_LAPLACE_GLM_MAX_CLASSES", L.LAPLACE_GLM_MAX_CLASSES), ("BNN_LAPLACE_GLM_MAX_LAYERS", L.LAPLACE_GLM_MAX_LAYERS),
             ("BNN_PREDICTIVE_MAX_QUANTILES", L.PREDICTIVE_MAX_QUANTILES), ("BNN_HIP_ABI_VERSION", L.ABI_VERSION)])
    _layout(tmp_path, L.LaplaceGlmFinishArgs, "bnn_laplace_glm_finish_args")
    _layout(tmp_path, L.LaplaceGlmSampleArgs, "bnn_laplace_glm_sample_args")
    assert L.LAPLACE_GLM_MAX_CLASSES == G.MAX_CLASSES == 16 and L.LAPLACE_GLM_MAX_LAYERS == L.LAPLACE_MAX_TENSORS // 2
    assert len(G.pairs(16)) == 136


# ---------------------------------------------------------------------------------------------- the documented error order
def _layer(**over):
    L = _L()
    d = dict(batch=4, rows=12, in_features=7, out_features=5, math=L.MATH_F32, gx_mask=1, precision=1.0)
    return _args(L.LaplaceGlmLayerArgs, ("x", "gy", "y", "w", "f_w", "f_b", "g_x", "cov_part", "v_out"), **dict(d, **over))


def _finish(**over):
    L = _L()
    d = dict(batch=4, classes=3, n_layers=2, mode=L.NLL_CLASSIFICATION, n_quantiles=0, n_samples=0, sigma=1.0,
             cov_part={0: FAKE, 1: FAKE}, tiles={0: 2, 1: 1})
    d = {k: ({**d[k], **v} if isinstance(v, dict) and isinstance(d.get(k), dict) else v) for k, v in {**d, **over}.items()}
    return _args(L.LaplaceGlmFinishArgs, ("mean", "cov", "var", "chol", "probs", "preds", "entropy", "predictive_variance",
                                          "quantiles"), **d)


def _sample(**over):
    L = _L()
    d = dict(n_samples=5, batch=4, classes=3, seed=7, sample_base=0)
    return _args(L.LaplaceGlmSampleArgs, ("mean", "chol", "logits"), **dict(d, **over))


def test_glm_layer_argument_errors():
    L = _L()
    _refused(L.load().bnn_laplace_glm_layer, _layer, C.sizeof(L.LaplaceGlmLayerArgs), [
        (SHAPE, (dict(batch=0), dict(rows=0), dict(in_features=0), dict(out_features=-1), dict(rows=13), dict(rows=4 * 17),
                 dict(rows=1 << 20, batch=1 << 16, in_features=1 << 12), dict(precision=0.0), dict(precision=float("nan")),
                 dict(precision=float("inf")), dict(precision=-1.0))),
        (ENUM, (dict(math=3), dict(math=-1))),
        (NULL, (dict(x=None), dict(gy=None), dict(f_w=None), dict(f_b=None), dict(cov_part=None), dict(w=None))),
        (ALIGN, (dict(x=FAKE + 2), dict(y=FAKE + 1), dict(f_b=FAKE + 2), dict(g_x=FAKE + 2), dict(cov_part=FAKE + 2), dict(v_out=FAKE + 3),
                 dict(precision_device=FAKE + 4))),
    ])
    # a device word makes the host value irrelevant; shape errors come before enum errors, enum before NULL, NULL before alignment
    fn = L.load().bnn_laplace_glm_layer
    assert fn(C.byref(_layer(precision=0.0, precision_device=FAKE, x=None)), None) == NULL
    assert fn(C.byref(_layer(rows=13, math=9, x=None)), None) == SHAPE
    assert fn(C.byref(_layer(math=9, x=None, y=FAKE + 1)), None) == ENUM
    assert fn(C.byref(_layer(x=None, y=FAKE + 1)), None) == NULL
    assert fn(C.byref(_layer(rows=4 * 16, g_x=None, w=None, x=FAKE + 1)), None) == ALIGN     # C = 16 is inside; w only with g_x


def test_glm_finish_argument_errors():
    L = _L()
    reg = dict(mode=L.NLL_REGRESSION)
    _refused(L.load().bnn_laplace_glm_finish, _finish, C.sizeof(L.LaplaceGlmFinishArgs), [
        (SHAPE, (dict(batch=0), dict(classes=0), dict(classes=17), dict(n_layers=0), dict(n_layers=L.LAPLACE_GLM_MAX_LAYERS + 1),
                 dict(tiles={1: 0}), dict(n_quantiles=-1), dict(n_quantiles=L.PREDICTIVE_MAX_QUANTILES + 1), dict(n_samples=-1),
                 dict(batch=1 << 24, classes=16), dict(sigma=0.0, **reg), dict(sigma=float("inf"), **reg),
                 dict(n_quantiles=1, z={0: float("nan")}, **reg))),
        (ENUM, (dict(mode=2), dict(mode=-1))),
        (NULL, (dict(cov_part={1: None}), dict(mean=None), dict(cov=None), dict(var=None), dict(chol=None),
                dict(n_quantiles=2, quantiles=None, **reg))),
        (ALIGN, (dict(cov_part={0: FAKE + 2}), dict(mean=FAKE + 2), dict(chol=FAKE + 1), dict(probs=FAKE + 2), dict(preds=FAKE + 4),
                 dict(entropy=FAKE + 2), dict(predictive_variance=FAKE + 2), dict(sample_counter=FAKE + 2))),
    ])
    fn = L.load().bnn_laplace_glm_finish
    assert fn(C.byref(_finish(sigma=0.0, mean=None)), None) == NULL            # (classification does not read sigma)
    assert fn(C.byref(_finish(classes=17, mode=5, mean=None)), None) == SHAPE
    assert fn(C.byref(_finish(mode=5, mean=None)), None) == ENUM
    assert fn(C.byref(_finish(mean=None, cov=FAKE + 2)), None) == NULL


def test_glm_sample_argument_errors():
    L = _L()
    _refused(L.load().bnn_laplace_glm_sample, _sample, C.sizeof(L.LaplaceGlmSampleArgs), [
        (SHAPE, (dict(n_samples=0), dict(batch=0), dict(classes=0), dict(classes=17), dict(n_samples=1 << 16, batch=1 << 14, classes=16))),
        (NULL, (dict(mean=None), dict(chol=None), dict(logits=None))),
        (ALIGN, (dict(mean=FAKE + 2), dict(chol=FAKE + 1), dict(logits=FAKE + 2), dict(sample_counter=FAKE + 2))),
    ])
    fn = L.load().bnn_laplace_glm_sample
    assert fn(C.byref(_sample(classes=17, mean=None)), None) == SHAPE
    assert fn(C.byref(_sample(mean=None, chol=FAKE + 2)), None) == NULL


def test_glm_host_side_refusals():
    import networks
    from bnn_hip import laplace, ops
    from bnn_hip.ops import BnnHipError

    class Stub:                                                  # the checks that need no device, on a bare object
        mode = "classification"

        class _Lin:
            out_features = 3
        layers = [type("D", (), dict(linear=_Lin))]
    s = Stub()
    with pytest.raises(BnnHipError, match="link must be one of"):
        laplace.DiagLaplace._glm_args(s, 0, "logit", None)
    with pytest.raises(BnnHipError, match="samples >= 1"):
        laplace.DiagLaplace._glm_args(s, 0, "mc", None)
    with pytest.raises(BnnHipError, match="regression summary"):
        laplace.DiagLaplace._glm_args(s, 0, "probit", [0.5])
    assert laplace.DiagLaplace._glm_args(s, 4, "mc", None) == ()
    Stub._Lin.out_features = 17
    with pytest.raises(BnnHipError, match="at most 16 outputs"):
        laplace.DiagLaplace._glm_args(s, 0, "probit", None)
    with pytest.raises(BnnHipError, match="positive and finite"):
        laplace.DiagLaplace._tau(s, 0.0, "glm_moments")
    with pytest.raises(BnnHipError, match="between 1 and 16 outputs"):
        ops.glm_pairs(17)
    assert ops.glm_pairs(16) == 136 and ops.glm_tiles(65) == 2 and ops.glm_tiles(64) == 1
    z = ops.normal_quantiles([0.0, 0.5, 0.975, 1.0])
    assert z[0] == -math.inf and z[3] == math.inf and z[1] == 0.0 and abs(z[2] - 1.959963984540054) < 1e-12
    with pytest.raises(BnnHipError):
        ops.normal_quantiles([1.5])
    with pytest.raises(BnnHipError):                             # CPU tensors: no fallback
        ops.laplace_glm_sample(torch.zeros(4, 3), torch.zeros(4, 3, 3), 2, seed=1)
    with pytest.raises(BnnHipError):
        ops.laplace_glm_finish([torch.zeros(1, 4, 6)], torch.zeros(4, 3), "classification")
    with pytest.raises(BnnHipError):
        ops.laplace_glm_layer(torch.zeros(4, 7), torch.zeros(12, 5), torch.zeros(5, 7), f_w=torch.zeros(5, 7), f_b=torch.zeros(5),
                              precision=1.0)
    mp = dict(input_shape=5, classes=3, batch_size=4, hidden_units=6, mode="classification")
    with pytest.raises(BnnHipError):
        networks.MLP(mp).laplace().glm_moments(torch.zeros(4, 1, 1, 5))


# ---------------------------------------------------------------------------------------------- the restatement itself
def _case(mode, dims=(7, 6, 6, 3), B=4, seed=11):
    weights = _net(seed, dims)
    rng = np.random.default_rng(seed + 1)
    x = rng.standard_normal((B, dims[0]))
    curv = [rng.uniform(0.0, 30.0, np.asarray(t).shape) for w, b in weights for t in (w, b)]
    return weights, curv, x


@pytest.mark.parametrize("mode", ["classification", "regression"])
@pytest.mark.parametrize("tau", [1e-2, 1.0, 50.0])
def test_restated_covariance_equals_the_jacobian_form(mode, tau):
    """7-6-6-3, batch 4: the layer-wise sum of gz gz' V against J diag(s^2) J^T from autograd Jacobians, rtol 1e-10."""
    weights, curv, x = _case(mode)
    mean, cov, parts = G.chain(weights, curv, tau, x)
    ref_mean, ref_cov = G.jacobian_cov(weights, curv, tau, x)
    np.testing.assert_allclose(mean, ref_mean, rtol=1e-12, atol=1e-14)
    assert np.abs(cov - ref_cov).max() <= 1e-10 * np.abs(ref_cov).max()
    np.testing.assert_allclose(cov, ref_cov, rtol=1e-10, atol=1e-10 * np.abs(ref_cov).max() * 1e-3)
    assert [p.shape for p in parts] == [(1, 4, 6)] * 3
    # Cov >= min s^2_b,last I: positive definite, and the finish stage's pieces
    floor = G.variance(curv[-1], tau).min()
    assert np.linalg.eigvalsh(cov).min() >= floor * (1 - 1e-9)
    out = G.finish(parts, mean, mode, sigma=0.7, levels=(0.0, 0.1, 0.5, 1.0))
    np.testing.assert_allclose(out["cov"], ref_cov, rtol=1e-10, atol=1e-13 * np.abs(ref_cov).max())
    L_ = out["chol"]
    assert np.isfinite(L_).all() and (np.triu(L_, 1) == 0).all() and (np.einsum("ncc->nc", L_) > 0).all()
    np.testing.assert_allclose(L_ @ L_.transpose(0, 2, 1), out["cov"], rtol=1e-12, atol=1e-14)
    if mode == "classification":
        want = torch.softmax(torch.tensor(mean) / torch.sqrt(1 + math.pi / 8 * torch.tensor(out["var"])), dim=1)
        np.testing.assert_allclose(out["probs"], want.numpy(), rtol=1e-13)
        np.testing.assert_allclose(out["entropy"], torch.distributions.Categorical(probs=want).entropy().numpy(), rtol=1e-12)
        assert (out["preds"] == want.argmax(dim=1).numpy()).all()
    else:
        np.testing.assert_allclose(out["predictive_variance"], out["var"] + 0.49, rtol=1e-15)
        q = out["quantiles"]
        assert (q[0] == -np.inf).all() and (q[3] == np.inf).all()
        np.testing.assert_allclose(q[2], mean, rtol=1e-15)
        nd = torch.distributions.Normal(torch.tensor(mean), torch.tensor(out["var"]).sqrt())
        np.testing.assert_allclose(nd.cdf(torch.tensor(q[1])).numpy(), 0.1, rtol=1e-9)


def test_masked_columns_are_left_out_not_multiplied():
    """A NaN V[n, o] reaches exactly the rows whose unit o is active."""
    rng = np.random.default_rng(5)
    B, Cc, out = 5, 3, 70
    gy = rng.standard_normal((B * Cc, out))
    y = rng.standard_normal((B, out))
    V = rng.uniform(0.1, 2.0, (B, out))
    V[:, 66] = np.nan
    part = G.layer_parts(gy, y, V, B)
    assert part.shape == (2, B, 6) and np.isfinite(part[0]).all()
    hit = np.isnan(part[1]).all(axis=1)
    assert (hit == (y[:, 66] > 0)).all() and 0 < hit.sum() < B
    assert np.isfinite(part[1][~hit]).all()
    bad = G.finish([part], np.zeros((B, Cc)), "classification")
    assert np.isnan(bad["chol"][hit][:, np.tri(Cc, dtype=bool)]).all() and np.isfinite(bad["chol"][~hit]).all()
    assert np.isnan(bad["probs"][hit]).all() and np.isfinite(bad["probs"][~hit]).all()


def test_fp32_chain_error_of_the_covariance_is_small_and_positive():
    weights, curv, x = _case("classification")
    _, cov, _ = G.chain(weights, curv, 1.0, x)
    err = np.abs(G.chain_torch32(weights, curv, 1.0, x).double().numpy() - cov).max() / np.abs(cov).max()
    assert 0 < err < 1e-5


# ---------------------------------------------------------------------------------------------- the sampler
def test_restated_eps_is_the_oracle_map_on_its_own_stream():
    from oracle import bnn_oracle as O
    e = G.glm_eps(2026, 3, 33, 10)
    assert e.shape == (33, 10) and e.dtype == np.float32 and np.isfinite(e).all()
    # the same group / slot map as philox_normal, another counter: equal shapes, different draws, and B does not enter
    assert not np.array_equal(e, O.philox_normal(2026, 5, 3, 33, 10))
    assert np.array_equal(G.glm_eps(2026, 3, 70, 10)[:33], e)
    assert not np.array_equal(G.glm_eps(2026, 4, 33, 10), e)
    # one element by hand: (n, j) = (7, 6) -> group 7 * 3 + 1, slot 2
    r = O.philox4x32(np.uint32(7 * 3 + 1), np.uint32(3), np.uint32(5), np.uint32(1), 2026, 0)
    assert O.box_muller(r[2], r[3])[0] == e[7, 6]


def test_restated_sampler_moments_at_4096_samples():
    """S = 4096 draws at a fixed (mean, chol): every sample mean and every sample covariance entry within 5 standard errors of
    (mean, cov); the standard error of a covariance entry of a Gaussian is sqrt((cov_ij^2 + cov_ii cov_jj) / S)."""
    rng = np.random.default_rng(21)
    B, Cc, S = 3, 5, 4096
    A = rng.standard_normal((B, Cc, Cc))
    cov = A @ A.transpose(0, 2, 1) + 0.3 * np.eye(Cc)
    chol = np.linalg.cholesky(cov)
    mean = rng.standard_normal((B, Cc))
    f, mag = G.sample(mean, chol, seed=99, first=1000, S=S)
    assert f.shape == (S, B, Cc) and (mag >= np.abs(f) - 1e-12).all()
    m = f.mean(axis=0)
    se_m = np.sqrt(np.einsum("ncc->nc", cov) / S)
    assert (np.abs(m - mean) <= 5 * se_m).all(), np.abs(m - mean) / se_m
    d = f - mean[None]
    sc = np.einsum("snc,snd->ncd", d, d) / S
    d2 = np.einsum("ncc->nc", cov)
    se_c = np.sqrt((cov ** 2 + d2[:, :, None] * d2[:, None, :]) / S)
    assert (np.abs(sc - cov) <= 5 * se_c).all(), (np.abs(sc - cov) / se_c).max()
    # a second call with the first index advanced by S continues the stream
    f2, _ = G.sample(mean, chol, seed=99, first=1000 + S // 2, S=S // 2)
    assert np.array_equal(f2, f[S // 2:])
