"""CPU-side checks of the diagonal Laplace posterior (bnn_laplace_*, bnn_hip.laplace; include/bnn_hip.h F17; no GPU): the entry
points exist and the ABI version is unchanged, the ctypes mirrors match the header, malformed arguments are refused on the host
with the documented status, and the fp64 restatement (tests/laplace_ref.py) equals an independent formulation -- per-row
Jacobians from autograd, the GGN from diag(p) - p p^T itself, the evidence from slogdet of the dense diagonal precision."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import laplace_ref as R
from test_bandit_cpu import _layout

FAKE = 0x10000
NEW = ("bnn_laplace_seed", "bnn_laplace_layer", "bnn_laplace_evidence", "bnn_laplace_posterior")
NULL, SHAPE, ENUM, WORKSPACE, ABI, ALIGN = -1, -2, -3, -4, -5, -6


def test_laplace_exports_and_abi_version():
    from bnn_hip import _lib as L
    lib = L.load()
    assert lib.bnn_version() == 9 == L.ABI_VERSION
    for name in NEW + ("bnn_laplace_evidence_workspace_bytes",):
        assert name in L.EXPORTS and hasattr(lib, name)
    import bnn_hip
    from bnn_hip import laplace, ops
    assert bnn_hip.DiagLaplace is laplace.DiagLaplace
    for name in ("laplace_seed", "laplace_layer", "laplace_evidence", "laplace_posterior"):
        assert callable(getattr(ops, name))
    import networks
    assert callable(networks.MLP.laplace) and callable(networks.MLP_Dropout.laplace)
    header = open(_layout.__globals__["HEADER"]).read()
    for name in NEW:
        assert f"int {name}(const {name}_args* args, void* stream);" in header
    assert "F17" in header


def test_laplace_struct_layouts_match_the_header(tmp_path):
    from bnn_hip import _lib as L
    _layout(tmp_path, L.LaplaceSeedArgs, "bnn_laplace_seed_args",
            [("BNN_LAPLACE_MAX_PRECISIONS", L.LAPLACE_MAX_PRECISIONS), ("BNN_LAPLACE_MAX_TENSORS", L.LAPLACE_MAX_TENSORS),
             ("BNN_LAPLACE_CHUNK", L.LAPLACE_CHUNK), ("BNN_LAPLACE_RECORD_DOUBLES", L.LAPLACE_RECORD_DOUBLES),
             ("BNN_LAPLACE_GGN", L.LAPLACE_GGN), ("BNN_LAPLACE_EMPIRICAL", L.LAPLACE_EMPIRICAL), ("BNN_HIP_ABI_VERSION", L.ABI_VERSION)])
    _layout(tmp_path, L.LaplaceLayerArgs, "bnn_laplace_layer_args")
    _layout(tmp_path, L.LaplaceEvidenceArgs, "bnn_laplace_evidence_args")
    _layout(tmp_path, L.LaplacePosteriorArgs, "bnn_laplace_posterior_args")
    assert L.LAPLACE_MAX_PRECISIONS >= 33                      # the default grid of fit_prior_precision fits one pass


def _args(cls, ptrs, **over):
    a = cls()
    a.struct_bytes = C.sizeof(cls)
    for f in ptrs:
        setattr(a, f, FAKE)
    for k, v in over.items():
        if isinstance(v, dict):                                # an array field: {index: value}
            for i, x in v.items():
                getattr(a, k)[i] = x
        else:
            setattr(a, k, v)
    return a


def _merge(d, over):
    """d updated by over; an array field ({index: value}) is updated entry by entry."""
    out = dict(d)
    for k, v in over.items():
        out[k] = {**out[k], **v} if isinstance(v, dict) and isinstance(out.get(k), dict) else v
    return out


def _seed(**over):
    from bnn_hip import _lib as L
    d = dict(batch=4, classes=3, loss_mode=L.NLL_CLASSIFICATION, curvature=L.LAPLACE_GGN, sigma=1.0)
    return _args(L.LaplaceSeedArgs, ("logits", "target", "gy", "record"), **dict(d, **over))


def _layer(**over):
    from bnn_hip import _lib as L
    d = dict(batch=4, rows=12, in_features=7, out_features=5, math=L.MATH_F32, gx_mask=1)
    return _args(L.LaplaceLayerArgs, ("x", "gy", "y", "w", "f_w", "f_b", "g_x", "s_out"), **dict(d, **over))


def _tensors(n=2):
    return dict(param={i: FAKE for i in range(n)}, curv={i: FAKE for i in range(n)}, numel={0: 5000, 1: 7})


def _evid(**over):
    d = dict(n_tensors=2, n_precisions=3, precision={0: 0.1, 1: 1.0, 2: 10.0}, workspace_bytes=1 << 20, **_tensors())
    return _args(_L().LaplaceEvidenceArgs, ("record", "workspace", "log_evidence", "best_index", "best"), **_merge(d, over))


def _post(**over):
    d = dict(n_tensors=2, precision=1.0, mu={0: FAKE, 1: FAKE}, rho={0: FAKE, 1: FAKE}, **_tensors())
    return _args(_L().LaplacePosteriorArgs, (), **_merge(d, over))


def _L():
    from bnn_hip import _lib as L
    return L


def _refused(fn, make, size, cases):
    """Every malformed call returns its documented status on the host (a NULL stream and fake pointers are never reached)."""
    assert fn(None, None) == NULL
    for delta in (8, -8):
        assert fn(C.byref(make(struct_bytes=size + delta)), None) == ABI
    for st, bads in cases:
        for bad in bads:
            assert fn(C.byref(make(**bad)), None) == st, bad
            assert fn(C.byref(make(struct_bytes=size + 8, **bad)), None) == ABI


def test_seed_argument_errors():
    L = _L()
    _refused(L.load().bnn_laplace_seed, _seed, C.sizeof(L.LaplaceSeedArgs), [
        (SHAPE, (dict(batch=0), dict(classes=0), dict(batch=-3), dict(sigma=0.0), dict(sigma=float("nan")), dict(sigma=float("inf")),
                 dict(batch=1 << 20, classes=1 << 10))),
        (ENUM, (dict(curvature=2), dict(curvature=-1), dict(loss_mode=2))),
        (NULL, (dict(logits=None), dict(gy=None), dict(record=None), dict(curvature=L.LAPLACE_EMPIRICAL, target=None))),
        (ALIGN, (dict(logits=FAKE + 2), dict(gy=FAKE + 1), dict(record=FAKE + 4), dict(target=FAKE + 4))),
    ])


def test_layer_argument_errors():
    L = _L()
    _refused(L.load().bnn_laplace_layer, _layer, C.sizeof(L.LaplaceLayerArgs), [
        (SHAPE, (dict(batch=0), dict(rows=0), dict(in_features=0), dict(out_features=-1), dict(rows=13),
                 dict(rows=1 << 20, batch=1 << 10, in_features=1 << 12))),
        (ENUM, (dict(math=3), dict(math=-1))),
        (NULL, (dict(x=None), dict(gy=None), dict(f_w=None), dict(w=None))),
        (ALIGN, (dict(x=FAKE + 2), dict(y=FAKE + 1), dict(f_b=FAKE + 2), dict(g_x=FAKE + 2), dict(s_out=FAKE + 3))),
    ])


def test_evidence_argument_errors():
    L = _L()
    lib = L.load()
    need = lib.bnn_laplace_evidence_workspace_bytes(C.byref(_evid()))
    assert need == (2 + 1) * (3 + 1) * 8                       # 5000 elements are two chunks, 7 one; G + 1 sums per block
    too_many = L.LAPLACE_MAX_PRECISIONS + 1
    assert lib.bnn_laplace_evidence_workspace_bytes(C.byref(_evid(n_precisions=too_many))) == 0
    _refused(lib.bnn_laplace_evidence, _evid, C.sizeof(L.LaplaceEvidenceArgs), [
        (SHAPE, (dict(n_precisions=too_many), dict(n_precisions=0), dict(n_tensors=0), dict(n_tensors=L.LAPLACE_MAX_TENSORS + 1),
                 dict(numel={1: 0}), dict(precision={1: 0.0}), dict(precision={2: -1.0}), dict(precision={0: float("inf")}))),
        (NULL, (dict(param={1: None}), dict(curv={0: None}), dict(record=None), dict(log_evidence=None))),
        (WORKSPACE, (dict(workspace=None), dict(workspace_bytes=need - 1))),
        (ALIGN, (dict(param={0: FAKE + 2}), dict(record=FAKE + 4), dict(workspace=FAKE + 4), dict(best=FAKE + 4), dict(best_index=FAKE + 2))),
    ])


def test_posterior_argument_errors():
    L = _L()
    _refused(L.load().bnn_laplace_posterior, _post, C.sizeof(L.LaplacePosteriorArgs), [
        (SHAPE, (dict(n_tensors=0), dict(n_tensors=L.LAPLACE_MAX_TENSORS + 1), dict(numel={0: -1}), dict(precision=0.0),
                 dict(precision=float("nan")))),
        (NULL, (dict(mu={1: None}), dict(rho={0: None}), dict(param={0: None}), dict(curv={1: None}))),
        (ALIGN, (dict(rho={1: FAKE + 2}), dict(precision_device=FAKE + 4))),
    ])


def test_host_side_refusals():
    import networks
    from bnn_hip import ops
    from bnn_hip.ops import BnnHipError
    mp = dict(input_shape=5, classes=3, batch_size=4, hidden_units=6, mode="classification")
    drop = networks.MLP_Dropout(mp)
    with pytest.raises(BnnHipError, match="dropout is on"):
        drop.laplace()
    with pytest.raises(BnnHipError, match="curvature"):
        networks.MLP(mp).laplace(curvature="kfac")
    with pytest.raises(BnnHipError, match="sigma"):
        networks.MLP(mp).laplace(sigma=0.0)
    with pytest.raises(BnnHipError):
        networks.MLP(mp).laplace()                              # CPU parameters: no fallback
    with pytest.raises(BnnHipError, match="candidate precisions"):
        ops.laplace_evidence([torch.zeros(3)], [torch.zeros(3)], np.logspace(-4, 4, 65), record=torch.zeros(2, dtype=torch.float64))
    assert ops.laplace_rows(4, 3, "ggn") == 12 and ops.laplace_rows(4, 3, "empirical") == 4


# ---------------------------------------------------------------------------------------------- the restatement itself
def _net(seed, dims):
    rng = np.random.default_rng(seed)
    return [(rng.uniform(-0.6, 0.6, (o, i)), rng.uniform(-0.3, 0.3, o)) for i, o in zip(dims[:-1], dims[1:])]


def _flat(tensors):
    return np.concatenate([np.asarray(t).reshape(-1) for t in tensors])


@pytest.mark.parametrize("mode,curvature", [("classification", "ggn"), ("classification", "empirical"), ("regression", "ggn"),
                                            ("regression", "empirical")])
def test_restated_curvature_equals_the_jacobian_form(mode, curvature):
    """5-6-6-3, batch 4: the staged product-of-squares form against diag(sum_n J_n^T H_n J_n) / sum_n (J_n^T d_n)^2."""
    weights = _net(3, (5, 6, 6, 3))
    rng = np.random.default_rng(4)
    x = rng.standard_normal((4, 5))
    y = rng.integers(0, 3, 4) if mode == "classification" else rng.standard_normal((4, 3))
    sigma = 0.7
    got, ll = R.accumulate(weights, x, y, mode, curvature, sigma)
    want = R.jacobian_curvature(weights, x, y, mode, curvature, sigma)
    g = _flat(got)
    assert g.shape == want.shape and (want > 0).any()
    assert np.abs(g - want).max() <= 1e-12 * np.abs(want).max()
    # the data term: log softmax / the Gaussian log density, by torch
    z = torch.tensor(R.forward(weights, x)[-1])
    if mode == "classification":
        ref_ll = -torch.nn.functional.cross_entropy(z, torch.tensor(y), reduction="sum").item()
    else:
        ref_ll = torch.distributions.Normal(z, sigma).log_prob(torch.tensor(y)).sum().item()
    assert abs(ll - ref_ll) <= 1e-12 * abs(ref_ll)


def test_restated_stage_shapes_and_the_virtual_row_order():
    rng = np.random.default_rng(9)
    z = rng.standard_normal((4, 3))
    gy, _ = R.seed(z, None, "classification", "ggn")
    p = R.softmax(z)
    assert gy.shape == (12, 3)
    for c in range(3):
        for n in range(4):
            e = np.eye(3)[c]
            np.testing.assert_allclose(gy[c * 4 + n], math.sqrt(p[n, c]) * (e - p[n]), rtol=1e-14, atol=1e-16)
    # sum over the virtual rows of a data row of the outer products is diag(p) - p p^T
    for n in range(4):
        H = sum(np.outer(gy[c * 4 + n], gy[c * 4 + n]) for c in range(3))
        np.testing.assert_allclose(H, np.diag(p[n]) - np.outer(p[n], p[n]), rtol=1e-13, atol=1e-16)
    gy_bad, ll_bad = R.seed(z, np.array([0, 3, 1, -1]), "classification", "ggn")
    assert np.isnan(ll_bad) and np.isnan(gy_bad.reshape(3, 4, 3)[:, [1, 3]]).all() and np.isfinite(gy_bad.reshape(3, 4, 3)[:, [0, 2]]).all()


def test_restated_evidence_equals_the_dense_log_determinant():
    weights = _net(5, (5, 6, 6, 3))
    rng = np.random.default_rng(6)
    x, y = rng.standard_normal((4, 5)), rng.integers(0, 3, 4)
    curv, ll = R.accumulate(weights, x, y, "classification", "ggn")
    params = [t for w, b in weights for t in (w, b)]
    taus = np.logspace(-4, 4, 9)
    got = R.evidence(params, curv, taus, ll)
    for g, t in zip(got, taus):
        want = R.dense_evidence(params, curv, t, ll)
        assert abs(g - want) <= 1e-12 * abs(want)
    i, gap = R.best_precision(got)
    assert i == int(np.argmax(got)) and gap > 0


def test_restated_posterior_round_trip():
    f = np.array([0.0, 1e-8, 1.0, 3e5, 1e12])
    for tau in (1e-4, 1.0, 1e4, 1e12):
        s = R.posterior_sigma(f, tau)
        np.testing.assert_allclose(s, 1.0 / np.sqrt(f + tau), rtol=1e-15)
        rho = R.inv_softplus(s)
        assert np.isfinite(rho).all()
        np.testing.assert_allclose(R.softplus(rho), s, rtol=1e-12)


def test_fp32_chain_error_is_small_and_positive():
    weights = _net(7, (5, 6, 6, 3))
    rng = np.random.default_rng(8)
    xs = [rng.standard_normal((4, 5)) for _ in range(2)]
    ys = [rng.integers(0, 3, 4) for _ in range(2)]
    err, ref = R.fp32_chain_error(weights, xs, ys, "classification", "ggn")
    assert 0 < err < 1e-5 and len(ref) == 6
