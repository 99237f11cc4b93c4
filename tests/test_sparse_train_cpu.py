"""CPU-side checks of the F14 sparse training step (bnn_sparse_elbo_terms, bnn_sparse_bwd, bnn_sparse_sigma_refresh,
posthoc.CompressedNetwork.parameters / graphed_train_step; no GPU): the entry points exist, the ctypes mirrors match the
header, every argument check runs on the host before a launch, the host API refuses what it must, and the restatement of
tests/sparse_train_ref.py is checked against itself: the closed forms against fp64 autograd (a check of the specification,
both sides fp64 with the same formula -- not a measurement), level 0 against the unmasked dense formula, and for every case
the GPU test uses that the comparison cannot be vacuous, together with the case's REF32."""
import ctypes as C

import numpy as np
import pytest
import torch

import sparse_train_ref as R
from oracle import bnn_oracle as O
from test_bandit_cpu import _layout

FAKE = 0x10000
NEW = ("bnn_sparse_elbo_terms_workspace_bytes", "bnn_sparse_elbo_terms", "bnn_sparse_bwd_workspace_bytes", "bnn_sparse_bwd",
       "bnn_sparse_sigma_refresh")


# ------------------------------------------------------------------------------------------------- exports and layouts
def test_sparse_train_exports():
    from bnn_hip import _lib as L, ops, posthoc, sparse_train
    lib = L.load()
    assert lib.bnn_version() == L.ABI_VERSION == 9
    for name in NEW:
        assert name in L.EXPORTS and hasattr(lib, name)
    for fn in (ops.sparse_elbo_terms, ops.sparse_elbo_terms_args, ops.sparse_bwd, ops.sparse_bwd_args, ops.sparse_sigma_refresh,
               ops.sparse_sigma_args, posthoc.CompressedNetwork.parameters, posthoc.CompressedNetwork.graphed_train_step,
               sparse_train.SparseTrainStep, sparse_train.csc_view):
        assert callable(fn)


def test_sparse_train_struct_layouts_match_the_header(tmp_path):
    from bnn_hip import _lib as L
    _layout(tmp_path, L.SparseElboLayer, "bnn_sparse_elbo_layer", [("BNN_SPARSE_MAX_LAYERS", L.SPARSE_MAX_LAYERS),
                                                                   ("BNN_SPARSE_MAX_SEGMENTS", L.SPARSE_MAX_SEGMENTS)])
    _layout(tmp_path, L.SparseElboArgs, "bnn_sparse_elbo_args")
    _layout(tmp_path, L.SparseBwdArgs, "bnn_sparse_bwd_args")
    _layout(tmp_path, L.SparseSigmaArgs, "bnn_sparse_sigma_args")


# ------------------------------------------------------------------------------------------------- argument validation
LAYER_PTRS = ("row_ptr", "col", "mu_val", "sigma_val", "b_mu", "b_sigma", "b_keep")


def _elbo_args(layer_over=None, **over):
    from bnn_hip import _lib as L
    a = L.SparseElboArgs()
    a.struct_bytes = C.sizeof(L.SparseElboArgs)
    a.n_layers, a.n_samples = 2, 3
    a.prior = L.Prior(L.PRIOR_GAUSS, 1.0, 0.5, 1.0, 0.0025)
    for i, (fin, fout, nnz) in enumerate(((70, 130, 4000), (130, 10, 0))):
        y = a.layer[i]
        y.in_features, y.out_features, y.nnz, y.layer_id = fin, fout, nnz, i
        for f in LAYER_PTRS:
            setattr(y, f, FAKE)
    a.log_prior = a.log_q = a.workspace = FAKE
    a.workspace_bytes = 1 << 20
    for k, v in (layer_over or {}).items():
        setattr(a.layer[1], k, v)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_elbo_terms_argument_validation_without_a_device():
    """Fake, never dereferenced device addresses: every rejection happens before a launch."""
    from bnn_hip import _lib as L
    lib = L.load()
    fn = lib.bnn_sparse_elbo_terms
    assert fn(None, None) == -1                                                            # BNN_ERR_NULL
    assert fn(C.byref(_elbo_args(struct_bytes=8)), None) == -5                             # BNN_ERR_ABI
    for bad in (dict(n_layers=0), dict(n_layers=9), dict(n_samples=0), dict(n_samples=65536)):
        assert fn(C.byref(_elbo_args(**bad)), None) == -2, bad                             # BNN_ERR_SHAPE
    for bad in (dict(in_features=0), dict(in_features=65537), dict(out_features=0), dict(nnz=-1), dict(nnz=1301)):
        assert fn(C.byref(_elbo_args(layer_over=bad)), None) == -2, bad
    assert fn(C.byref(_elbo_args(prior=L.Prior(2, 1.0, 0.5, 1.0, 1.0))), None) == -3       # BNN_ERR_ENUM
    assert fn(C.byref(_elbo_args(prior=L.Prior(L.PRIOR_GAUSS, 0.0, 0.5, 1.0, 1.0))), None) == -2
    assert fn(C.byref(_elbo_args(prior=L.Prior(L.PRIOR_MIXTURE, 1.0, 0.5, 1.0, 0.0))), None) == -2
    for f in ("log_prior", "log_q"):
        assert fn(C.byref(_elbo_args(**{f: None})), None) == -1, f
    for f in LAYER_PTRS:
        assert fn(C.byref(_elbo_args(layer_over={f: None})), None) == -1, f
    assert fn(C.byref(_elbo_args(workspace=None)), None) == -4                             # BNN_ERR_WORKSPACE
    nnz, outs = (C.c_int32 * 2)(4000, 0), (C.c_int32 * 2)(130, 10)
    need = lib.bnn_sparse_elbo_terms_workspace_bytes(2, 3, nnz, outs)
    assert need == (4 + 1 + 0 + 1) * 3 * 16                   # blocks of 1024 entries and of 256 biases, a float4 per sample
    assert fn(C.byref(_elbo_args(workspace_bytes=need - 1)), None) == -4
    assert lib.bnn_sparse_elbo_terms_workspace_bytes(0, 3, nnz, outs) == 0 == lib.bnn_sparse_elbo_terms_workspace_bytes(2, 0, nnz, outs)
    for f, off in (("workspace", 8), ("log_prior", 2), ("log_q", 2), ("sample_counter", 2)):
        assert fn(C.byref(_elbo_args(**{f: FAKE + off})), None) == -6, f                   # BNN_ERR_ALIGN
    for f, off in (("row_ptr", 2), ("col", 1), ("mu_val", 2), ("sigma_val", 2), ("b_mu", 2), ("b_sigma", 1)):
        assert fn(C.byref(_elbo_args(layer_over={f: FAKE + off})), None) == -6, f


BWD_PTRS = ("row_ptr", "col", "mu_val", "rho_val", "b_mu", "b_rho", "b_keep", "x", "gy", "g_mu_val", "g_rho_val", "g_b_mu", "g_b_rho",
            "workspace")


def _bwd_args(**over):
    from bnn_hip import _lib as L
    a = L.SparseBwdArgs()
    a.struct_bytes = C.sizeof(L.SparseBwdArgs)
    a.n_samples, a.rows, a.in_features, a.out_features, a.nnz = 3, 37, 70, 130, 4000
    a.prior = L.Prior(L.PRIOR_MIXTURE, 1.0, 0.5, 1.0, 0.0025)
    for f in BWD_PTRS:
        setattr(a, f, FAKE)
    a.workspace_bytes = 1 << 20
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_backward_argument_validation_without_a_device():
    from bnn_hip import _lib as L
    lib = L.load()
    fn = lib.bnn_sparse_bwd
    assert fn(None, None) == -1
    assert fn(C.byref(_bwd_args(struct_bytes=0)), None) == -5
    for bad in (dict(n_samples=0), dict(n_samples=65536), dict(rows=0), dict(in_features=0), dict(in_features=65537),
                dict(out_features=0), dict(nnz=-1), dict(nnz=9101), dict(x_per_sample=-1),
                dict(out_features=65537, g_x=FAKE, col_ptr=FAKE, row=FAKE, perm=FAKE),     # uint16 rows in the CSC view
                dict(rows=65535 * 256 + 1, g_x=FAKE, col_ptr=FAKE, row=FAKE, perm=FAKE)):  # the input gradient's grid
        assert fn(C.byref(_bwd_args(**bad)), None) == -2, bad
    assert fn(C.byref(_bwd_args(prior=L.Prior(-1, 1.0, 0.5, 1.0, 1.0))), None) == -3
    assert fn(C.byref(_bwd_args(prior=L.Prior(L.PRIOR_MIXTURE, 1.0, 0.5, 0.0, 1.0))), None) == -2
    assert fn(C.byref(_bwd_args(prior=L.Prior(L.PRIOR_GAUSS, -1.0, 0.5, 1.0, 1.0))), None) == -2
    for f in BWD_PTRS[:-1]:
        assert fn(C.byref(_bwd_args(**{f: None})), None) == -1, f
    assert fn(C.byref(_bwd_args(relu=1)), None) == -1                                      # y missing
    for miss in ("col_ptr", "row", "perm"):                                                # the CSC view with g_x
        kw = dict(g_x=FAKE, col_ptr=FAKE, row=FAKE, perm=FAKE)
        kw[miss] = None
        assert fn(C.byref(_bwd_args(**kw)), None) == -1, miss
    need = lib.bnn_sparse_bwd_workspace_bytes(3, 37, 130)
    assert need == 3 * 37 * 130 * 4 and lib.bnn_sparse_bwd_workspace_bytes(0, 37, 130) == 0
    for gz in (dict(gy_row_major=1), dict(relu=1, y=FAKE)):                                # the gz launch needs the workspace ...
        assert fn(C.byref(_bwd_args(workspace=None, **gz)), None) == -4
        assert fn(C.byref(_bwd_args(workspace_bytes=need - 4, **gz)), None) == -4
    assert fn(C.byref(_bwd_args(workspace=None, workspace_bytes=0, row_ptr=FAKE + 2)), None) == -6   # ... nobody else: on to the next check
    for f, off in (("row_ptr", 2), ("col", 1), ("mu_val", 2), ("rho_val", 2), ("col_ptr", 2), ("row", 1), ("perm", 2), ("b_mu", 2),
                   ("b_rho", 2), ("x", 2), ("y", 2), ("gy", 1), ("g_log_prior", 2), ("g_log_q", 2), ("g_mu_val", 2), ("g_rho_val", 2),
                   ("g_b_mu", 2), ("g_b_rho", 2), ("g_x", 2), ("workspace", 2), ("sample_counter", 2)):
        kw = {f: FAKE + off}
        if f == "g_x":
            kw.update(col_ptr=FAKE, row=FAKE, perm=FAKE)
        assert fn(C.byref(_bwd_args(**kw)), None) == -6, f


def _sigma_args(**over):
    from bnn_hip import _lib as L
    a = L.SparseSigmaArgs()
    a.struct_bytes = C.sizeof(L.SparseSigmaArgs)
    a.n_segments = 2
    for i in range(2):
        a.rho[i], a.sigma[i], a.n[i] = FAKE, FAKE, 100
    a.keep[1] = FAKE
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_sigma_refresh_argument_validation_without_a_device():
    from bnn_hip import _lib as L
    fn = L.load().bnn_sparse_sigma_refresh
    assert fn(None, None) == -1
    assert fn(C.byref(_sigma_args(struct_bytes=16)), None) == -5
    for bad in (0, 9, -1):
        assert fn(C.byref(_sigma_args(n_segments=bad)), None) == -2, bad
    for f in ("rho", "sigma"):
        a = _sigma_args()
        getattr(a, f)[1] = None
        assert fn(C.byref(a), None) == -1, f
        a = _sigma_args()
        getattr(a, f)[0] = FAKE + 2
        assert fn(C.byref(a), None) == -6, f
    a = _sigma_args()
    a.n[1] = -1
    assert fn(C.byref(a), None) == -2
    a = _sigma_args()                                                                      # nothing to do: no launch, no error
    a.n[0] = a.n[1] = 0
    a.rho[0] = None
    assert fn(C.byref(a), None) == 0


# ------------------------------------------------------------------------------------------------- host API
def _hand_made_network(nnz=(2, 1, 1), kept_bias=True, prior=None):
    """A CompressedNetwork of CPU tensors, built by hand: 3-4-4-2."""
    from bnn_hip import posthoc
    layers = []
    for i, ((fin, fout), n) in enumerate(zip(((3, 4), (4, 4), (4, 2)), nnz)):
        c = posthoc._CsrLayer()
        c.fin, c.fout, c.nnz, c.layer_id = fin, fout, n, i
        c.row_ptr = torch.tensor([0] + [n] * fout, dtype=torch.int32)
        c.col = torch.zeros(max(n, 1), dtype=torch.int16)
        c.mu_val, c.rho_val = torch.full((max(n, 1),), 0.1), torch.full((max(n, 1),), -4.0)
        c.sigma_val = torch.log1p(torch.exp(c.rho_val))
        c.b_mu = torch.full((fout,), 0.05 if kept_bias else 0.0)
        c.b_rho = torch.full((fout,), -4.0 if kept_bias else 0.0)
        c.b_sigma = torch.log1p(torch.exp(c.b_rho)) if kept_bias else torch.zeros(fout)
        c.mu_sign = c.rho_sign = None
        layers.append(c)
    return posthoc.CompressedNetwork(layers, "classification", False, prior=prior)


def test_parameters_share_storage_in_the_stated_order():
    cn = _hand_made_network(nnz=(2, 0, 1))
    ps = cn.parameters()
    assert len(ps) == 12 and all(isinstance(p, torch.nn.Parameter) and p.dtype == torch.float32 for p in ps)
    for i, c in enumerate(cn._layers):
        mu, rho, bmu, brho = ps[4 * i:4 * i + 4]
        assert tuple(mu.shape) == tuple(rho.shape) == (c.nnz,) and tuple(bmu.shape) == tuple(brho.shape) == (c.fout,)
        for p, t in ((mu, c.mu_val), (rho, c.rho_val), (bmu, c.b_mu), (brho, c.b_rho)):
            assert p.untyped_storage().data_ptr() == t.untyped_storage().data_ptr() and p.storage_offset() == t.storage_offset()
    with torch.no_grad():
        ps[0].add_(1.0)
        ps[11].mul_(2.0)
    assert torch.equal(cn._layers[0].mu_val[:2], torch.full((2,), 1.1)) and torch.equal(cn._layers[2].b_rho, torch.full((2,), -8.0))
    again = cn.parameters()
    assert all(a is b for a, b in zip(ps, again))                                          # created once, cached
    assert cn.prior is None
    assert sorted(cn.state_dict()) == sorted(f"l{i}.{k}" for i in (1, 2, 3) for k in ("row_ptr", "col", "mu_val", "rho_val", "bias_mu", "bias_rho"))


def test_graphed_train_step_refuses_what_cannot_run():
    from bnn_hip import ops
    from bnn_hip.ops import BnnHipError
    from bnn_hip.optim import FusedAdam
    from bnn_hip.runtime import state
    x, y = torch.zeros(5, 3), torch.zeros(5, dtype=torch.int64)
    prior = ops.PriorSpec(False, 1.0)
    cn = _hand_made_network()
    cap = FusedAdam(cn.parameters(), lr=1e-3, capturable=True)
    with pytest.raises(BnnHipError, match="no prior"):
        cn.graphed_train_step(cap, x, y, 2)
    with pytest.raises(BnnHipError, match="capturable"):
        cn.graphed_train_step(FusedAdam(cn.parameters(), lr=1e-3), x, y, 2, prior=prior)
    host = state.host_eps
    state.host_eps = True
    try:
        with pytest.raises(BnnHipError, match="eps"):
            cn.graphed_train_step(cap, x, y, 2, prior=prior)
    finally:
        state.host_eps = host
    dead = _hand_made_network(nnz=(0, 0, 0), kept_bias=False, prior=prior)
    with pytest.raises(BnnHipError, match="no survivor"):
        dead.graphed_train_step(FusedAdam(dead.parameters(), lr=1e-3, capturable=True), x, y, 2)
    with pytest.raises(BnnHipError, match="no CPU fallback"):                              # everything else needs the device
        _hand_made_network(prior=prior).graphed_train_step(cap, x, y, 2)


def test_csc_view_is_a_stable_sort_of_col():
    from bnn_hip.sparse_train import csc_view
    rs = np.random.RandomState(3)
    keep = rs.rand(9, 7) < 0.4
    keep[:, 2] = False                                                                     # an empty column
    keep[4] = False                                                                        # an empty row
    r, c = np.nonzero(keep)
    rp = torch.tensor(np.concatenate([[0], np.cumsum(np.bincount(r, minlength=9))]), dtype=torch.int32)
    col_ptr, row, perm = csc_view(rp, torch.tensor(c, dtype=torch.int16), len(c), 7)
    assert col_ptr.dtype == torch.int32 and row.dtype == torch.int16 and perm.dtype == torch.int32
    rt, ct = np.nonzero(keep.T)                                                            # column-major order: (column, row)
    np.testing.assert_array_equal(col_ptr.numpy(), np.concatenate([[0], np.cumsum(np.bincount(rt, minlength=7))]))
    np.testing.assert_array_equal(row.numpy()[:len(c)], ct)
    np.testing.assert_array_equal(r[perm.numpy()[:len(c)]], ct)
    np.testing.assert_array_equal(c[perm.numpy()[:len(c)]], rt)
    assert col_ptr[3] == col_ptr[2]


# ------------------------------------------------------------------------------------------------- the restatement itself
def _scale_check(a, b, tol, what):
    assert R.rel_dev(a, b) <= tol, (what, R.rel_dev(a, b))


@pytest.mark.parametrize("mixture", [False, True])
@pytest.mark.parametrize("mode,dims", [("classification", (9, 7, 4)), ("regression", (5, 6, 1))])
def test_closed_forms_agree_with_fp64_autograd(mode, dims, mixture):
    case = R.build_case(dims, mode, False, .5, 11, 3, mixture=mixture, first=4)
    case["layers"][1]["b_keep"][:] = 0                                                     # a layer without any kept bias
    for k in ("b_mu", "b_rho", "b_sigma"):
        case["layers"][1][k] = np.zeros_like(case["layers"][1][k])
    o_a, g_a = R.autograd_ref(case)
    o_c, g_c = R.closed_ref(case, np.float64)
    _scale_check(o_c, o_a, 1e-12, "out4")
    for name, a, b in zip(R.GRAD_NAMES, g_c, g_a):
        assert a.shape == b.shape
        _scale_check(a, b, 1e-12, name)
    assert not g_c[6].any() and not g_c[7].any()                                           # a pruned bias receives no gradient


def test_level_0_is_the_unmasked_dense_formula():
    """Everything kept: the step's ELBO is networks.py:73-88 + :205-208 term for term (the oracle's restatement in fp64)."""
    from bnn_hip import synth
    dims, rows, S, beta = (9, 7, 4), 11, 2, 0.3
    sd = synth.synth_state_dict(*dims, False)
    params = [(sd[f"{n}.weight_mu"], sd[f"{n}.weight_rho"], sd[f"{n}.bias_mu"], sd[f"{n}.bias_rho"]) for n in ("l1", "l2", "l3")]
    exact = lambda rho: np.log1p(np.exp(np.asarray(rho, dtype=np.float64)))
    layers = R.layers_from_dense(params, [np.ones_like(p[0], dtype=bool) for p in params], [np.ones_like(p[2], dtype=bool) for p in params],
                                 sigma=exact)
    x, y = synth.synth_batch("classification", rows, dims[0], dims[2], seed=5)
    for mixture in (False, True):
        prior = dict(mixture=mixture, sigma_p=1.0, pi=0.5, sigma1=1.0, sigma2=np.exp(-6.0))
        case = dict(layers=layers, x=x.reshape(rows, -1), y=y, mode="classification", S=S, first=2, seed=2026, beta=beta, prior=prior,
                    nll_sigma=1.0)
        out4, _ = R.closed_ref(case, np.float64)
        p = O.NetParams([tuple(torch.tensor(np.asarray(t, dtype=np.float64)) for t in q) for q in params], "classification", dims[0],
                        False, O.Prior(mixture, 1.0, 0.5, 1.0, float(np.exp(-6.0))))
        lps, lqs, nl = [], [], 0.0
        for s in range(S):
            eps = [torch.tensor(e) for l in layers for e in R.dense_eps(2026, l["layer_id"], 2 + s, l["fout"], l["fin"])]
            out, lp, lq = O.network_forward(p, torch.tensor(x.reshape(rows, -1), dtype=torch.float64), eps)
            lps.append(float(lp))
            lqs.append(float(lq))
            nl += float(O.nll(out, torch.tensor(y), "classification"))
        want = np.array([beta * np.mean(lqs) - beta * np.mean(lps) + nl / S, np.mean(lps), np.mean(lqs), nl / S])
        np.testing.assert_allclose(out4, want, rtol=1e-12)


# 1-48-1 at 98 %: about 50 of 2497 parameters survive, one of them in layer 1 and one in layer 3, and no path from the input to
# the output is left whatever the parameter seed (seeds 1 .. 7 were tried): the data term of every gradient is exactly zero
# there, and what the GPU comparison checks in that case is the complexity term (regenerated epsilon, the prior, log q).
DATA_DEAD = (2,)


@pytest.mark.parametrize("ci", range(len(R.CASES)))
def test_every_gpu_case_has_live_gradients_and_a_small_ref32(ci):
    """For the cases tests/test_gpu_sparse_train.py uses (restated pattern): the reference gradient has a non-zero entry in
    g_mu and g_rho of every layer with survivors -- also with beta = 0, i.e. through the data term alone, so a dead-ReLU case
    cannot make the GPU comparison vacuous -- and REF32 leaves the GPU test's tolerance 4 x REF32 under the 2e-4 it may not
    exceed."""
    dims, mode, lr, level, rows, S, mixture = R.CASES[ci]
    case = R.build_case(dims, mode, lr, level, rows, S, mixture=mixture)
    ref = R.closed_ref(case, np.float64)
    data_only = R.closed_ref(dict(case, beta=0.0), np.float64)[1]
    for i, l in enumerate(case["layers"]):
        if len(l["col"]):
            assert np.any(ref[1][4 * i] != 0) and np.any(ref[1][4 * i + 1] != 0), (ci, i)
            live = np.any(data_only[4 * i] != 0) and np.any(data_only[4 * i + 1] != 0)
            assert live != (ci in DATA_DEAD), (ci, i, "data term")
    r32 = R.ref32_of(case, ref)
    print(f"case {ci} {R.CASES[ci]}: nnz {[len(l['col']) for l in case['layers']]} REF32 {r32:.3e}")
    assert 4 * r32 <= 2e-4
