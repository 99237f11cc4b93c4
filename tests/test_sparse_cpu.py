"""CPU-side checks of the F13 compressed network (bnn_sparse_count, bnn_sparse_fill, bnn_sparse_fwd,
posthoc.CompressedNetwork; no GPU): the entry points exist, the ctypes mirrors match the header, every argument check runs
on the host before a launch, the size formula, and the fp64 restatement and the error bound the GPU tests use -- kept in
this file.

The bound.  The kernel computes, per output element, acc_k = fl(fma(x_k, w_k, acc_(k-1))) for k = 1 .. n (acc_0 = 0) and
y = fl(acc_n + b): n + 1 roundings in a chain, each a factor (1 + d), |d| <= u = 2^-24.  The standard running-error bound
of such a chain (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1: the inner product) is
|y - (sum_k x_k w_k + b)| <= gamma(n + 1) (sum_k |x_k w_k| + |b|), gamma(k) = k u / (1 - k u).  Under sampling the weight
itself, w_k = fl(fma(sigma_k, eps_k, mu_k)), carries one more rounding against the fp64 restatement's sigma eps + mu (and
so does the bias): gamma(n + 2).  chain_bound returns that, so the single-layer tolerance is derived, not chosen."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_bandit_cpu import _layout
from test_prune_sweep_cpu import codes_ref, thresholds_ref

FAKE = 0x10000
U = 2.0 ** -24


# ------------------------------------------------------------------------------------------------- the fp64 restatement
def csr_ref(code, p):
    """(row_ptr int32 [out + 1], col uint16 [nnz], rows int64 [nnz]) of the survivors code > p of a [out, in] code array,
    row by row, columns ascending (np.nonzero's order)."""
    code = np.asarray(code)
    r, c = np.nonzero(code > p)
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=code.shape[0]))]).astype(np.int32)
    return row_ptr, c.astype(np.uint16), r.astype(np.int64)


def _rows_of(row_ptr):
    return np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))


def sparse_layer_ref(layer, x, eps=None):
    """One layer in float64 over the kept entries only.  layer: dict(row_ptr, col, mu_val, sigma_val, b_mu, b_sigma, fin);
    eps: None (the mean weights) or (eps_w [nnz], eps_b [out]).  Returns (pre-activation [rows, out], w [nnz], b [out])."""
    rp, col = np.asarray(layer["row_ptr"]), np.asarray(layer["col"]).astype(np.int64)
    w = np.asarray(layer["mu_val"], dtype=np.float64)
    b = np.asarray(layer["b_mu"], dtype=np.float64)
    if eps is not None:
        w = w + np.asarray(layer["sigma_val"], dtype=np.float64) * np.asarray(eps[0], dtype=np.float64)
        b = b + np.asarray(layer["b_sigma"], dtype=np.float64) * np.asarray(eps[1], dtype=np.float64)
    out = len(rp) - 1
    W = np.zeros((out, int(layer["fin"])))
    W[_rows_of(rp), col] = w
    return np.asarray(x, dtype=np.float64) @ W.T + b, w, b


def sparse_forward_ref(layers, x, eps=None):
    """fp64 outputs [rows, classes] of the compressed network: ReLU between the layers; eps: None or one (eps_w, eps_b)
    per layer (one MC sample)."""
    h = np.asarray(x, dtype=np.float64).reshape(len(x), -1)
    for i, layer in enumerate(layers):
        h, _, _ = sparse_layer_ref(layer, h, None if eps is None else eps[i])
        if i + 1 < len(layers):
            h = np.maximum(h, 0.0)
    return h


def gamma(k):
    return k * U / (1.0 - k * U)


def chain_bound(x, w, b):
    """gamma(n + 2) (sum_j |x_j w_j| + |b|) for one output: x [..., n], w [n], b a scalar."""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    return gamma(w.shape[-1] + 2) * (np.abs(x * w).sum(-1) + abs(float(b)))


def chain_bound_layer(x, row_ptr, col, w, b):
    """chain_bound of every output [rows, out] of a CSR layer (w, b: the fp64 weights and biases the restatement used)."""
    x = np.asarray(x, dtype=np.float64)
    out = len(row_ptr) - 1
    bound = np.empty((x.shape[0], out))
    for o in range(out):
        lo, hi = int(row_ptr[o]), int(row_ptr[o + 1])
        bound[:, o] = chain_bound(x[:, np.asarray(col[lo:hi], dtype=np.int64)], w[lo:hi], b[o])
    return bound


# ------------------------------------------------------------------------------------------------- exports and layouts
NEW = ("bnn_sparse_count", "bnn_sparse_fill", "bnn_sparse_fwd")


def test_sparse_exports():
    from bnn_hip import _lib as L, ops, posthoc
    lib = L.load()
    assert lib.bnn_version() == L.ABI_VERSION == 9
    for name in NEW:
        assert name in L.EXPORTS and hasattr(lib, name)
    for fn in (ops.sparse_count, ops.sparse_fill, ops.sparse_fwd, ops.sparse_fwd_args, posthoc.compress, posthoc.PruneSweep.compress,
               posthoc.CompressedNetwork.forward, posthoc.CompressedNetwork.forward_mc, posthoc.CompressedNetwork.to_dense):
        assert callable(fn)


def test_sparse_struct_layouts_match_the_header(tmp_path):
    from bnn_hip import _lib as L
    _layout(tmp_path, L.SparseCountArgs, "bnn_sparse_count_args", [("BNN_HIP_ABI_VERSION", L.ABI_VERSION)])
    _layout(tmp_path, L.SparseFillArgs, "bnn_sparse_fill_args")
    _layout(tmp_path, L.SparseFwdArgs, "bnn_sparse_fwd_args")


# ------------------------------------------------------------------------------------------------- argument validation
def _args(cls, fields, pointers, **over):
    a = cls()
    a.struct_bytes = C.sizeof(cls)
    for k, v in fields.items():
        setattr(a, k, v)
    for f in pointers:
        setattr(a, f, FAKE)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _count_args(**over):
    from bnn_hip import _lib as L
    return _args(L.SparseCountArgs, dict(out_features=10, in_features=20, ld=32, level=1), ("code", "row_ptr"), **over)


def test_count_argument_validation_without_a_device():
    """Fake, never dereferenced device addresses: every rejection happens before a launch."""
    from bnn_hip import _lib as L
    fn = L.load().bnn_sparse_count
    assert fn(None, None) == -1                                                            # BNN_ERR_NULL
    assert fn(C.byref(_count_args(struct_bytes=4)), None) == -5                            # BNN_ERR_ABI
    for bad in (dict(out_features=0), dict(in_features=0), dict(ld=19), dict(level=-1), dict(level=L.PRUNE_MAX_LEVELS),
                dict(out_features=1 << 16, in_features=1 << 15, ld=1 << 15)):
        assert fn(C.byref(_count_args(**bad)), None) == -2, bad                            # BNN_ERR_SHAPE
    for f in ("code", "row_ptr"):
        assert fn(C.byref(_count_args(**{f: None})), None) == -1, f
    assert fn(C.byref(_count_args(row_ptr=FAKE + 2)), None) == -6                          # BNN_ERR_ALIGN


FILL_PTRS = ("code", "row_ptr", "mu", "rho", "col", "mu_val", "rho_val")


def _fill_args(**over):
    from bnn_hip import _lib as L
    return _args(L.SparseFillArgs, dict(out_features=10, in_features=20, ld=32, level=0, transposed=0), FILL_PTRS, **over)


def test_fill_argument_validation_without_a_device():
    from bnn_hip import _lib as L
    fn = L.load().bnn_sparse_fill
    assert fn(None, None) == -1
    assert fn(C.byref(_fill_args(struct_bytes=C.sizeof(L.SparseFillArgs) + 8)), None) == -5
    for bad in (dict(out_features=0), dict(in_features=-3), dict(ld=19), dict(level=-1), dict(level=16),
                dict(in_features=65537, ld=65600)):                                        # uint16 columns
        assert fn(C.byref(_fill_args(**bad)), None) == -2, bad
    assert fn(C.byref(_fill_args(in_features=65536, ld=65536, code=None)), None) == -1     # 65536 columns still fit
    for f in FILL_PTRS:
        assert fn(C.byref(_fill_args(**{f: None})), None) == -1, f
    for f, off in (("row_ptr", 2), ("mu", 2), ("rho", 1), ("mu_val", 2), ("rho_val", 2), ("col", 1)):
        assert fn(C.byref(_fill_args(**{f: FAKE + off})), None) == -6, f


FWD_PTRS = ("row_ptr", "col", "mu_val", "sigma_val", "b_mu", "b_sigma", "x", "y")


def _fwd_args(**over):
    from bnn_hip import _lib as L
    return _args(L.SparseFwdArgs, dict(n_samples=3, rows=37, in_features=70, out_features=130, eps_mode=L.EPS_PHILOX, relu=1,
                                       x_per_sample=0), FWD_PTRS, **over)


def test_forward_argument_validation_without_a_device():
    from bnn_hip import _lib as L
    fn = L.load().bnn_sparse_fwd
    assert fn(None, None) == -1
    assert fn(C.byref(_fwd_args(struct_bytes=0)), None) == -5
    for bad in (dict(n_samples=0), dict(n_samples=65536), dict(rows=0), dict(in_features=0), dict(in_features=65537),
                dict(out_features=-1), dict(x_per_sample=-1)):
        assert fn(C.byref(_fwd_args(**bad)), None) == -2, bad
    for code in (3, -1):
        assert fn(C.byref(_fwd_args(eps_mode=code)), None) == -3, code                     # BNN_ERR_ENUM
    for f in FWD_PTRS:
        assert fn(C.byref(_fwd_args(**{f: None})), None) == -1, f
    for f in ("sigma_val", "b_sigma"):                                                     # the mean forward needs no sigma ...
        assert fn(C.byref(_fwd_args(eps_mode=L.EPS_ZERO, row_ptr=None, **{f: None})), None) == -1, f   # (... row_ptr it does)
    assert fn(C.byref(_fwd_args(eps_mode=L.EPS_MEMORY)), None) == -1                       # eps, eps_b missing
    assert fn(C.byref(_fwd_args(eps_mode=L.EPS_MEMORY, eps=FAKE)), None) == -1
    for f, off in (("row_ptr", 2), ("col", 1), ("mu_val", 2), ("sigma_val", 2), ("b_mu", 2), ("b_sigma", 1), ("x", 2), ("y", 2),
                   ("eps_dump", 2), ("eps_b_dump", 2), ("x_scratch", 2), ("sample_counter", 2)):
        assert fn(C.byref(_fwd_args(**{f: FAKE + off})), None) == -6, f


def test_host_api_rejects_what_cannot_run():
    from bnn_hip import ops, posthoc
    from bnn_hip.ops import BnnHipError
    with pytest.raises(BnnHipError, match="BayesianNetwork"):
        posthoc.compress(torch.nn.Linear(2, 2), 0.5)
    with pytest.raises(BnnHipError, match="no CPU fallback"):
        ops.sparse_count(torch.zeros((4, 32), dtype=torch.uint8), 0, torch.zeros(5, dtype=torch.int32), out_features=4, in_features=20)


# ------------------------------------------------------------------------------------------------- sizes
def test_state_bytes_formula():
    """Per layer: row_ptr 4 (out + 1), col 2 nnz, mu_val and rho_val 4 nnz each, the two masked bias vectors 4 out each, and
    with zero_signs one bit per dense weight for each of mu and rho."""
    from bnn_hip.posthoc import compressed_state_bytes
    shapes = [(784, 1200), (1200, 1200), (1200, 10)]
    nnzs = [18816, 28800, 240]
    want = sum(4 * (o + 1) + 2 * n + 4 * n + 4 * n + 4 * o + 4 * o for (_, o), n in zip(shapes, nnzs))
    assert compressed_state_bytes(shapes, nnzs, zero_signs=False) == want == 507492
    signs = sum(2 * ((i * o + 7) // 8) for i, o in shapes)
    assert compressed_state_bytes(shapes, nnzs, zero_signs=True) == want + signs == want + 598200
    assert compressed_state_bytes([(7, 3)], [0], zero_signs=True) == 4 * 4 + 8 * 3 + 2 * 3
    dense = 4 * 2 * sum(i * o + o for i, o in shapes)                                      # the 19.2 MB of a prune_weights copy
    assert dense == 19161680 and compressed_state_bytes(shapes, nnzs) < dense / 17


# ------------------------------------------------------------------------------------------------- the restatement itself
def test_csr_restatement_agrees_with_the_level_codes():
    rs = np.random.RandomState(11)
    snr = (rs.standard_normal((13, 70)) * 12 + 5).astype(np.float32)
    snr[4] = -np.inf                                                                       # a row pruned at every level
    levels = (0., .5, .98, 1.)
    thr = thresholds_ref(snr, levels)
    code = codes_ref(snr, thr)
    for p, t in enumerate(thr):
        row_ptr, col, rows = csr_ref(code, p)
        assert row_ptr.dtype == np.int32 and col.dtype == np.uint16 and row_ptr[0] == 0
        with np.errstate(invalid="ignore"):
            keep = snr > np.float32(t)
        assert row_ptr[-1] == keep.sum() == len(col)
        for o in range(13):
            assert np.array_equal(col[row_ptr[o]:row_ptr[o + 1]], np.flatnonzero(keep[o]))
            assert np.all(rows[row_ptr[o]:row_ptr[o + 1]] == o)
        assert row_ptr[5] == row_ptr[4]                                                    # the empty row
    assert csr_ref(code, len(levels) - 1)[0][-1] == 0                                      # level 1.0: nothing survives


def test_forward_restatement_and_bound():
    rs = np.random.RandomState(5)
    W = rs.uniform(-1, 1, (6, 9))
    code = rs.randint(0, 3, (6, 9)).astype(np.uint8)
    code[2] = 0
    rp, col, rows = csr_ref(code, 0)
    layer = dict(row_ptr=rp, col=col, mu_val=W[rows, col], sigma_val=np.full(len(col), 0.5), b_mu=rs.uniform(-1, 1, 6),
                 b_sigma=np.full(6, 0.25), fin=9)
    x = rs.uniform(0, 1, (4, 9))
    y, w, b = sparse_layer_ref(layer, x)
    np.testing.assert_allclose(y, x @ np.where(code > 0, W, 0).T + layer["b_mu"], rtol=1e-14)
    np.testing.assert_array_equal(y[:, 2], np.broadcast_to(layer["b_mu"][2], 4))          # an empty row is its bias
    eps = (rs.standard_normal(len(col)), rs.standard_normal(6))
    ys, ws, bs = sparse_layer_ref(layer, x, eps)
    np.testing.assert_allclose(ws, layer["mu_val"] + 0.5 * eps[0], rtol=1e-15)
    np.testing.assert_allclose(bs, layer["b_mu"] + 0.25 * eps[1], rtol=1e-15)
    bound = chain_bound_layer(x, rp, col, w, b)
    assert bound.shape == (4, 6)
    n0 = rp[1] - rp[0]
    assert bound[1, 0] == chain_bound(x[1, col[:n0].astype(int)], w[:n0], b[0])
    assert np.isclose(gamma(3), 3 * U, rtol=1e-6) and np.all(bound[:, 2] == gamma(2) * abs(b[2]))
    code2 = rs.randint(0, 2, (3, 6)).astype(np.uint8)
    rp2, col2, rows2 = csr_ref(code2, 0)
    W2 = rs.uniform(-1, 1, (3, 6))
    layer2 = dict(row_ptr=rp2, col=col2, mu_val=W2[rows2, col2], sigma_val=np.zeros(len(col2)), b_mu=np.zeros(3), b_sigma=np.zeros(3), fin=6)
    two = sparse_forward_ref([layer, layer2], x)
    np.testing.assert_allclose(two, np.maximum(y, 0) @ np.where(code2 > 0, W2, 0).T, rtol=1e-14, atol=1e-15)
