"""CPU-side checks of the Kronecker-factored Laplace posterior (bnn_kfac_*, bnn_hip.kfac; include/bnn_hip.h F20; no GPU): the
entry points exist and the ABI version is unchanged, the ctypes mirrors match the header, malformed arguments are refused on
the host with the documented status in the documented order, the host-side refusals, and the fp64 restatement
(tests/kfac_ref.py) against an independent formulation -- factors from autograd Jacobians, the dense kron(G, Abar) / N + tau I,
its slogdet and solve, M M^T = P^-1 for the sampling map, and the exactness of the Kronecker form for N = 1."""
import ctypes as C

import numpy as np
import pytest
import torch

import kfac_ref as K
import laplace_ref as R
from test_bandit_cpu import _layout
from test_laplace_cpu import _args, _merge, _refused

FAKE = 0x10000
NEW = ("bnn_kfac_layer", "bnn_kfac_evidence", "bnn_kfac_glm_rotate", "bnn_kfac_glm_var", "bnn_kfac_sample")
NULL, SHAPE, ENUM, WORKSPACE, ABI, ALIGN = -1, -2, -3, -4, -5, -6


def _L():
    from bnn_hip import _lib as L
    return L


def test_kfac_exports_and_abi_version():
    L = _L()
    lib = L.load()
    assert lib.bnn_version() == 9 == L.ABI_VERSION
    for name in NEW + ("bnn_kfac_evidence_workspace_bytes", "bnn_kfac_sample_workspace_bytes"):
        assert name in L.EXPORTS and hasattr(lib, name)
    import bnn_hip
    from bnn_hip import kfac, laplace, ops
    assert bnn_hip.KronLaplace is kfac.KronLaplace and "KronLaplace" in bnn_hip.__all__
    assert issubclass(kfac.KronLaplace, laplace.LaplaceBase) and issubclass(laplace.DiagLaplace, laplace.LaplaceBase)
    assert not hasattr(kfac.KronLaplace, "network") and hasattr(laplace.DiagLaplace, "network")
    for name in ("kfac_layer", "kfac_evidence", "kfac_glm_rotate", "kfac_glm_var", "kfac_sample"):
        assert callable(getattr(ops, name))
    header = open(_layout.__globals__["HEADER"]).read()
    for name in NEW:
        assert f"int {name}(const {name}_args* args, void* stream);" in header
    assert "F20" in header and "#define BNN_HIP_ABI_VERSION 9" in header and "#define BNN_EPS_MAP_VERSION 2" in header
    assert L.KFAC_NOISE_WORD3 == K.NOISE_WORD3 == 4


def test_kfac_struct_layouts_match_the_header(tmp_path):
    L = _L()
    _layout(tmp_path, L.KfacLayerArgs, "bnn_kfac_layer_args", [("BNN_LAPLACE_GLM_MAX_LAYERS", L.LAPLACE_GLM_MAX_LAYERS),
                                                               ("BNN_HIP_ABI_VERSION", L.ABI_VERSION)])
    _layout(tmp_path, L.KfacEvidenceArgs, "bnn_kfac_evidence_args")
    _layout(tmp_path, L.KfacGlmRotateArgs, "bnn_kfac_glm_rotate_args")
    _layout(tmp_path, L.KfacGlmVarArgs, "bnn_kfac_glm_var_args")
    _layout(tmp_path, L.KfacSampleArgs, "bnn_kfac_sample_args")


# ------------------------------------------------------------------------------------------------ C-ABI refusals, in order
def _layer(**over):
    L = _L()
    d = dict(batch=4, rows=12, in_features=7, out_features=5, math=L.MATH_F32, gx_mask=1)
    return _args(L.KfacLayerArgs, ("x", "gy", "y", "w", "a", "s", "g", "g_x"), **dict(d, **over))


def _evid(**over):
    two = {0: FAKE, 1: FAKE}
    d = dict(n_layers=2, n_precisions=3, precision={0: 0.1, 1: 1.0, 2: 10.0}, workspace_bytes=1 << 20, weight=two, bias=two,
             lambda_a=two, lambda_g=two, in_features={0: 99, 1: 6}, out_features={0: 50, 1: 1})
    return _args(_L().KfacEvidenceArgs, ("record", "workspace", "log_evidence", "best_index", "best"), **_merge(d, over))


def _rotate(**over):
    L = _L()
    d = dict(batch=4, rows=12, in_features=7, out_features=5, math=L.MATH_F32, gx_mask=1)
    return _args(L.KfacGlmRotateArgs, ("x", "gy", "y", "w", "q_a", "q_g", "at", "gt", "g_x"), **dict(d, **over))


def _var(**over):
    d = dict(batch=4, rows=12, in_features=7, out_features=5, precision=1.0)
    return _args(_L().KfacGlmVarArgs, ("at", "gt", "lambda_a", "lambda_g", "cov_part", "v_out"), **dict(d, **over))


def _sample(**over):
    d = dict(members=3, first=0, in_features=7, out_features=5, layer=1, seed=5, precision=1.0, bank_stride=128, w_offset=0,
             b_offset=64, workspace_bytes=3 * 5 * 8 * 4)
    return _args(_L().KfacSampleArgs, ("w", "b", "q_a", "q_g", "lambda_a", "lambda_g", "bank", "workspace"), **dict(d, **over))


def test_kfac_layer_argument_errors():
    L = _L()
    _refused(L.load().bnn_kfac_layer, _layer, C.sizeof(L.KfacLayerArgs), [
        (SHAPE, (dict(batch=0), dict(rows=0), dict(in_features=0), dict(out_features=-1), dict(rows=13),
                 dict(rows=1 << 20, batch=1 << 10, in_features=1 << 12), dict(in_features=1 << 16), dict(out_features=1 << 16),
                 dict(batch=0, math=7), dict(rows=13, x=None))),            # (the shape is judged before the enum and the pointers)
        (ENUM, (dict(math=3), dict(math=-1), dict(math=3, x=None))),
        (NULL, (dict(x=None), dict(gy=None), dict(a=None), dict(s=None), dict(g=None), dict(w=None), dict(x=None, gy=FAKE + 2))),
        (ALIGN, (dict(x=FAKE + 2), dict(y=FAKE + 1), dict(a=FAKE + 2), dict(s=FAKE + 2), dict(g=FAKE + 2), dict(g_x=FAKE + 2))),
    ])


def test_kfac_evidence_argument_errors():
    L = _L()
    lib = L.load()
    need = lib.bnn_kfac_evidence_workspace_bytes(C.byref(_evid()))
    assert need == (2 + 1) * (3 + 1) * 8                       # 50 x 100 elements are two chunks, 1 x 7 one; G + 1 sums per block
    too_many = L.LAPLACE_MAX_PRECISIONS + 1
    assert lib.bnn_kfac_evidence_workspace_bytes(C.byref(_evid(n_precisions=too_many))) == 0
    assert lib.bnn_kfac_evidence_workspace_bytes(C.byref(_evid(in_features={1: 0}))) == 0
    _refused(lib.bnn_kfac_evidence, _evid, C.sizeof(L.KfacEvidenceArgs), [
        (SHAPE, (dict(n_precisions=too_many), dict(n_precisions=0), dict(n_layers=0), dict(n_layers=L.LAPLACE_GLM_MAX_LAYERS + 1),
                 dict(in_features={1: 0}), dict(out_features={0: -2}), dict(precision={1: 0.0}), dict(precision={2: -1.0}),
                 dict(precision={0: float("inf")}), dict(precision={0: 0.0}, record=None))),
        (NULL, (dict(weight={1: None}), dict(bias={0: None}), dict(lambda_a={0: None}), dict(lambda_g={1: None}), dict(record=None),
                dict(log_evidence=None), dict(record=None, workspace=None))),
        (WORKSPACE, (dict(workspace=None), dict(workspace_bytes=need - 1), dict(workspace=None, record=FAKE + 4))),
        (ALIGN, (dict(weight={0: FAKE + 2}), dict(lambda_a={1: FAKE + 4}), dict(lambda_g={0: FAKE + 4}), dict(record=FAKE + 4),
                 dict(workspace=FAKE + 4), dict(best=FAKE + 4), dict(best_index=FAKE + 2))),
    ])


def test_kfac_glm_argument_errors():
    L = _L()
    lib = L.load()
    _refused(lib.bnn_kfac_glm_rotate, _rotate, C.sizeof(L.KfacGlmRotateArgs), [
        (SHAPE, (dict(batch=0), dict(rows=0), dict(in_features=0), dict(out_features=-1), dict(rows=13),
                 dict(rows=4 * (L.LAPLACE_GLM_MAX_CLASSES + 1)), dict(in_features=1 << 16), dict(out_features=1 << 16),
                 dict(rows=13, math=9))),
        (ENUM, (dict(math=3), dict(math=-1), dict(math=3, at=None))),
        (NULL, (dict(x=None), dict(gy=None), dict(q_a=None), dict(q_g=None), dict(at=None), dict(gt=None), dict(w=None))),
        (ALIGN, (dict(x=FAKE + 2), dict(y=FAKE + 1), dict(q_a=FAKE + 2), dict(q_g=FAKE + 2), dict(at=FAKE + 2), dict(gt=FAKE + 2),
                 dict(g_x=FAKE + 2))),
    ])
    _refused(lib.bnn_kfac_glm_var, _var, C.sizeof(L.KfacGlmVarArgs), [
        (SHAPE, (dict(batch=0), dict(rows=0), dict(in_features=0), dict(out_features=0), dict(rows=13),
                 dict(rows=4 * (L.LAPLACE_GLM_MAX_CLASSES + 1)), dict(precision=0.0), dict(precision=float("nan")),
                 dict(precision=float("inf")), dict(precision=0.0, at=None))),
        (NULL, (dict(at=None), dict(gt=None), dict(lambda_a=None), dict(lambda_g=None), dict(cov_part=None))),
        (ALIGN, (dict(at=FAKE + 2), dict(gt=FAKE + 2), dict(lambda_a=FAKE + 4), dict(lambda_g=FAKE + 4), dict(cov_part=FAKE + 2),
                 dict(v_out=FAKE + 2), dict(precision_device=FAKE + 4))),
    ])
    assert lib.bnn_kfac_glm_var(C.byref(_var(precision=0.0, precision_device=FAKE + 4)), None) == ALIGN   # the device word wins


def test_kfac_sample_argument_errors():
    L = _L()
    lib = L.load()
    assert lib.bnn_kfac_sample_workspace_bytes(3, 7, 5) == 3 * 5 * 8 * 4
    assert lib.bnn_kfac_sample_workspace_bytes(0, 7, 5) == 0 and lib.bnn_kfac_sample_workspace_bytes(3, 0, 5) == 0
    _refused(lib.bnn_kfac_sample, _sample, C.sizeof(L.KfacSampleArgs), [
        (SHAPE, (dict(members=0), dict(first=-1), dict(in_features=0), dict(out_features=0), dict(bank_stride=-1), dict(w_offset=-1),
                 dict(b_offset=-4), dict(in_features=1 << 16), dict(out_features=1 << 16), dict(precision=0.0),
                 dict(precision=float("nan")), dict(members=0, w=None))),
        (NULL, (dict(w=None), dict(b=None), dict(q_a=None), dict(q_g=None), dict(lambda_a=None), dict(lambda_g=None), dict(bank=None),
                dict(bank=None, workspace=None))),
        (WORKSPACE, (dict(workspace=None), dict(workspace_bytes=3 * 5 * 8 * 4 - 1), dict(workspace=None, w=FAKE + 2))),
        (ALIGN, (dict(w=FAKE + 2), dict(b=FAKE + 2), dict(q_a=FAKE + 1), dict(q_g=FAKE + 2), dict(lambda_a=FAKE + 4),
                 dict(lambda_g=FAKE + 4), dict(bank=FAKE + 2), dict(workspace=FAKE + 2), dict(precision_device=FAKE + 4))),
    ])


# ------------------------------------------------------------------------------------------------ the host side
def test_kfac_host_side_refusals(monkeypatch):
    import networks
    from bnn_hip import kfac, laplace, ops
    from bnn_hip.ops import BnnHipError
    mp = dict(input_shape=5, classes=3, batch_size=4, hidden_units=6, mode="classification")
    with pytest.raises(BnnHipError, match="KronLaplace: the network's dropout is on"):
        networks.MLP_Dropout(mp).laplace(structure="kron")
    with pytest.raises(BnnHipError, match="KronLaplace: curvature"):
        networks.MLP(mp).laplace(structure="kron", curvature="kfac")
    with pytest.raises(BnnHipError, match="KronLaplace: sigma"):
        networks.MLP(mp).laplace(structure="kron", sigma=0.0)
    with pytest.raises(BnnHipError):
        networks.MLP(mp).laplace(structure="kron")              # CPU parameters: no fallback
    with pytest.raises(BnnHipError, match="structure must be"):
        networks.MLP(mp).laplace(structure="full")
    # the structure only chooses the class: 'diag' (the default) is DiagLaplace as before, with the keywords passed on
    seen = []
    monkeypatch.setattr(laplace, "DiagLaplace", lambda mlp, **kw: seen.append(("diag", kw)) or "D")
    monkeypatch.setattr(kfac, "KronLaplace", lambda mlp, **kw: seen.append(("kron", kw)) or "K")
    m = networks.MLP(mp)
    assert m.laplace() == "D" and m.laplace(structure="diag", sigma=2.0) == "D" and m.laplace(structure="kron", curvature="empirical") == "K"
    assert seen == [("diag", {}), ("diag", dict(sigma=2.0)), ("kron", dict(curvature="empirical"))]
    monkeypatch.undo()
    # the checks of the shared GLM interface that need no device, on a bare object: the class's own name in the message
    Stub = type("KronLaplace", (), dict(mode="classification", layers=[type("D", (), dict(linear=type("Lin", (), dict(out_features=17))))]))
    with pytest.raises(BnnHipError, match="KronLaplace: the linearised predictive handles at most 16 outputs"):
        kfac.KronLaplace._glm_args(Stub(), 0, "probit", None)
    with pytest.raises(BnnHipError, match="KronLaplace.sample_bank: the prior precision must be positive"):
        kfac.KronLaplace._tau(Stub(), -1.0, "sample_bank")
    with pytest.raises(BnnHipError, match="members must be >= 1"):
        kfac.KronLaplace.sample_bank(Stub(), 0)
    with pytest.raises(BnnHipError, match="candidate precisions"):
        ops.kfac_evidence([torch.zeros(3, 2)], [torch.zeros(3)], [torch.zeros(3, dtype=torch.float64)], [torch.zeros(3, dtype=torch.float64)],
                          np.logspace(-4, 4, 65), record=torch.zeros(2, dtype=torch.float64))
    with pytest.raises(BnnHipError):                             # CPU tensors: no fallback
        ops.kfac_layer(torch.zeros(4, 5), torch.zeros(4, 3), torch.zeros(3, 5), a=torch.zeros(5, 5), s=torch.zeros(5), g=torch.zeros(3, 3))
    # members per launch: the byte budget of the widest layer's T, at least one, at most all
    lays = [type("D", (), dict(linear=type("Lin", (), dict(in_features=9, out_features=10)))),
            type("D", (), dict(linear=type("Lin", (), dict(in_features=10, out_features=3))))]
    s = type("S", (), dict(layers=lays))()
    assert kfac.KronLaplace.members_per_launch(s, 30, budget_bytes=400 * 7) == 7
    assert kfac.KronLaplace.members_per_launch(s, 30, budget_bytes=1) == 1 and kfac.KronLaplace.members_per_launch(s, 5) == 5


# ------------------------------------------------------------------------------------------------ the restatement itself
def _net(seed, dims):
    rng = np.random.default_rng(seed)
    return [(rng.uniform(-0.6, 0.6, (o, i)), rng.uniform(-0.3, 0.3, o)) for i, o in zip(dims[:-1], dims[1:])]


CASES = [("classification", (5, 4, 3), "ggn"), ("classification", (5, 4, 3), "empirical"), ("regression", (1, 6, 1), "ggn"),
         ("regression", (1, 6, 1), "empirical")]


def _data(mode, dims, n, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, dims[0]))
    y = rng.integers(0, dims[-1], n) if mode == "classification" else rng.standard_normal((n, dims[-1]))
    return x, y


def _fit(weights, mode, dims, curvature, sigma, n=6, seed=11):
    """Two minibatches of n / 2 rows through the restated stages: (factors, loglik, x, y)."""
    x, y = _data(mode, dims, n, seed)
    tot, ll = None, 0.0
    for a in (0, n // 2):
        inc, l = K.accumulate(weights, x[a:a + n // 2], y[a:a + n // 2], mode, curvature, sigma)
        tot, ll = K.add(tot, inc), ll + l
    return tot, ll, x, y


@pytest.mark.parametrize("mode,dims,curvature", CASES)
def test_restated_factors_equal_the_jacobian_form(mode, dims, curvature):
    weights, sigma = _net(3, dims), 0.7
    got, ll, x, y = _fit(weights, mode, dims, curvature, sigma)
    want = K.jacobian_factors(weights, x, y, mode, curvature, sigma)
    for (a, s, g), (wa, ws, wg) in zip(got, want):
        for u, v in ((a, wa), (s, ws), (g, wg)):
            assert u.shape == v.shape and np.abs(u - v).max() <= 1e-12 * max(np.abs(v).max(), 1e-300)
        assert np.array_equal(a, a.T) and np.abs(g - g.T).max() <= 1e-15 * np.abs(g).max()
    assert any(np.abs(g).max() > 0 for _, _, g in got)


@pytest.mark.parametrize("mode,dims,curvature", CASES[::2])
def test_restated_evidence_glm_and_sampling_equal_the_dense_kronecker_form(mode, dims, curvature):
    weights, sigma, N = _net(5, dims), 0.7, 6
    factors, ll, x, y = _fit(weights, mode, dims, curvature, sigma)
    decs = [K.decompose(a, s, g, N) for a, s, g in factors]
    taus = np.array([1e-2, 1.0, 1e2])
    ev = K.evidence(weights, [(d[1], d[3]) for d in decs], taus, ll)
    xt, _ = _data(mode, dims, 4, 12)
    for t, e in zip(taus, ev):
        want = K.dense_evidence(weights, factors, N, t, ll)
        assert abs(e - want) <= 1e-11 * abs(want)
        mean, cov = K.glm_cov(weights, xt, decs, t)
        ref = K.dense_glm_cov(weights, xt, factors, N, t)
        assert cov.shape == ref.shape == (4, dims[-1], dims[-1])
        assert np.abs(cov - ref).max() <= 1e-10 * np.abs(ref).max()
        np.testing.assert_allclose(mean, R.forward(weights, xt)[-1], rtol=0, atol=0)
        for (w, b), (a, s, g), (QA, lA, QG, lG) in zip(weights, factors, decs):
            M = K.sampling_map(QA, lA, QG, lG, t)
            P = K.dense_precision(a, s, g, N, t)
            assert np.abs(M @ M.T @ P - np.eye(P.shape[0])).max() <= 1e-9
            E = np.random.default_rng(13).standard_normal((w.shape[0], w.shape[1] + 1))
            ws, bs = K.sample(w, b, QA, lA, QG, lG, t, E)
            want_bar = np.concatenate([w, b[:, None]], axis=1).reshape(-1) + M @ E.reshape(-1)
            assert np.abs(np.concatenate([ws, bs[:, None]], axis=1).reshape(-1) - want_bar).max() <= 1e-12
    i, gap = R.best_precision(ev)
    assert i == int(np.argmax(ev)) and gap > 0


@pytest.mark.parametrize("mode,dims", [("classification", (5, 4, 3)), ("regression", (1, 6, 1))])
def test_the_kronecker_form_is_exact_for_one_row(mode, dims):
    """N = 1: kron(G, Abar) / N is the layer's full GGN block J^T H J, whatever the layer (Martens & Grosse's expectation
    approximation averages nothing)."""
    weights, sigma = _net(7, dims), 0.7
    x, y = _data(mode, dims, 1, 14)
    factors, _ = K.accumulate(weights, x, y, mode, "ggn", sigma)
    blocks = K.ggn_block(weights, x, mode, sigma)
    for (a, s, g), blk in zip(factors, blocks):
        k = np.kron(g, K.abar_of(a, s, 1.0))
        assert k.shape == blk.shape and np.abs(blk).max() > 0
        assert np.abs(k - blk).max() <= 1e-12 * np.abs(blk).max()
    # and with more rows it is an approximation: the same comparison must NOT hold (the test above would be vacuous otherwise)
    x6, y6 = _data(mode, dims, 6, 15)
    f6, _ = K.accumulate(weights, x6, y6, mode, "ggn", sigma)
    b6 = K.ggn_block(weights, x6, mode, sigma)
    a, s, g = f6[0]
    if dims[0] > 1:
        assert np.abs(np.kron(g, K.abar_of(a, s, 6.0)) / 6.0 - b6[0]).max() > 1e-6 * np.abs(b6[0]).max()


def test_restated_noise_stream():
    """Element e of Wbar draws slot e & 3 of the counter (e >> 2, sample, layer, 4): rows do not start new groups, another sample,
    layer or seed gives other values, and the draws are standard normal."""
    from oracle import bnn_oracle as O
    seed = 0x1234567890ABCDEF
    E = K.noise(seed, 7, 2, 5, 7)                                # [5, 7]: 35 elements, 9 groups
    r = O.philox4x32(np.uint32(33 >> 2), np.uint32(7), np.uint32(2), np.uint32(4), seed & 0xFFFFFFFF, seed >> 32)
    assert E[4, 5] == O.box_muller(r[0], r[1])[1]                 # element 33 = (4, 5): group 8, slot 1
    r = O.philox4x32(np.uint32(2), np.uint32(7), np.uint32(2), np.uint32(4), seed & 0xFFFFFFFF, seed >> 32)
    assert E[1, 3] == O.box_muller(r[2], r[3])[0]                 # element 10 = (1, 3): group 2, slot 2
    assert np.array_equal(K.noise(seed, 7, 2, 9, 7)[:5], E)      # more rows only append
    for other in (K.noise(seed, 8, 2, 5, 7), K.noise(seed, 7, 1, 5, 7), K.noise(seed + 1, 7, 2, 5, 7)):
        assert not np.array_equal(other, E)
    big = K.noise(seed, 0, 0, 200, 101)
    assert abs(big.mean()) < 0.02 and abs(big.std() - 1.0) < 0.02
