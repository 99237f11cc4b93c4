"""CPU-side checks of deep-ensemble training (bnn_ens_fwd, bnn_ens_loss, bnn_ens_bwd, bnn_hip.ensemble; include/bnn_hip.h F21;
no GPU): the entry points exist and the ABI version is unchanged, the ctypes mirrors match the header, malformed arguments
are refused on the host in the documented order (validation only: no call reaches a launch), the gradient bucket's views
follow bank_layout, and the seeded initialisation is reproducible, distinct per seed, reset_parameters() under that seed,
and leaves the network and the caller's generator alone.  (A WeightBank needs device parameters, so the bank half of the
seed test lives in tests/test_gpu_ensemble.py.)"""
import ctypes as C

import pytest
import torch

from test_bandit_cpu import _layout
from test_laplace_cpu import ABI, ALIGN, ENUM, FAKE, NULL, SHAPE, _args, _refused

NEW = ("bnn_ens_fwd", "bnn_ens_loss", "bnn_ens_bwd")


def _L():
    from bnn_hip import _lib as L
    return L


def test_ensemble_exports_and_abi_version():
    L = _L()
    lib = L.load()
    assert lib.bnn_version() == 9 == L.ABI_VERSION
    for name in NEW:
        assert name in L.EXPORTS and hasattr(lib, name)
    import bnn_hip
    import networks
    from bnn_hip import ensemble, ops
    assert bnn_hip.DeepEnsemble is ensemble.DeepEnsemble and bnn_hip.EnsembleTrainStep is ensemble.EnsembleTrainStep
    for name in ("ens_fwd", "ens_loss", "ens_bwd"):
        assert callable(getattr(ops, name))
    for name in ("parameters", "member", "state_dict", "load_state_dict", "graphed_train_step"):
        assert callable(getattr(ensemble.DeepEnsemble, name))
    assert callable(networks.MLP.ensemble) and callable(networks.MLP_Dropout.ensemble)
    header = open(_layout.__globals__["HEADER"]).read()
    for name in NEW:
        assert f"int {name}(const {name}_args* args, void* stream);" in header
    assert "F21" in header and "#define BNN_HIP_ABI_VERSION 9" in header


def test_ensemble_struct_layouts_match_the_header(tmp_path):
    L = _L()
    _layout(tmp_path, L.EnsFwdArgs, "bnn_ens_fwd_args", [("BNN_HIP_ABI_VERSION", L.ABI_VERSION)])
    _layout(tmp_path, L.EnsLossArgs, "bnn_ens_loss_args")
    _layout(tmp_path, L.EnsBwdArgs, "bnn_ens_bwd_args")
    _layout(tmp_path, L.BankFwdArgs, "bnn_bank_fwd_args")                       # the existing struct stays as it is


# ---------------------------------------------------------------------------------------------- the documented error order
def _fwd(**over):
    L = _L()
    d = dict(members=3, first=0, batch=5, in_features=37, out_features=10, x_shared=1, relu=1, math=L.MATH_F32, layer_id=1,
             w_stride=448, b_stride=448, drop_p=0.5, seed=7, sample_offset=11)
    return _args(L.EnsFwdArgs, ("x", "w", "b", "y", "sample_counter"), **dict(d, **over))


def _loss(**over):
    L = _L()
    d = dict(members=3, batch=5, classes=10, loss_mode=L.NLL_CLASSIFICATION, target_shared=1, grad_scale=1.0)
    return _args(L.EnsLossArgs, ("logits", "target", "loss", "g_logits"), **dict(d, **over))


def _bwd(**over):
    L = _L()
    d = dict(members=3, first=0, batch=5, in_features=37, out_features=10, x_shared=0, math=L.MATH_BF16, gx_mask=1,
             y_scale=2.0, gx_scale=2.0, w_stride=448, g_stride=448)
    return _args(L.EnsBwdArgs, ("x", "gy", "y", "w", "g_w", "g_b", "g_x"), **dict(d, **over))


def test_ens_fwd_argument_errors():
    L = _L()
    fn = L.load().bnn_ens_fwd
    _refused(fn, _fwd, C.sizeof(L.EnsFwdArgs), [
        (SHAPE, (dict(members=0), dict(members=-2), dict(first=-1), dict(batch=0), dict(in_features=0), dict(out_features=-2),
                 dict(layer_id=-1), dict(w_stride=-1), dict(b_stride=-1), dict(drop_p=1.0), dict(drop_p=-0.1),
                 dict(drop_p=float("nan")), dict(sample_counter_inc=3), dict(members=1 << 20, batch=1 << 20, out_features=64))),
        (ENUM, (dict(math=3), dict(math=-1))),
        (NULL, (dict(x=None), dict(w=None), dict(y=None), dict(drop_p=0.0, sample_counter_inc=3, sample_counter=None))),
        (ALIGN, (dict(x=FAKE + 2), dict(w=FAKE + 1), dict(b=FAKE + 2), dict(y=FAKE + 3), dict(sample_counter=FAKE + 2))),
    ])
    # shape before enum, enum before NULL, NULL before alignment; no bias and no counter are not errors
    assert fn(C.byref(_fwd(batch=0, math=9, x=None)), None) == SHAPE
    assert fn(C.byref(_fwd(math=9, x=None, y=FAKE + 1)), None) == ENUM
    assert fn(C.byref(_fwd(x=None, y=FAKE + 1)), None) == NULL
    assert fn(C.byref(_fwd(b=None, sample_counter=None, y=FAKE + 1)), None) == ALIGN


def test_ens_loss_argument_errors():
    L = _L()
    fn = L.load().bnn_ens_loss
    _refused(fn, _loss, C.sizeof(L.EnsLossArgs), [
        (SHAPE, (dict(members=0), dict(batch=0), dict(classes=-1), dict(batch=1 << 20, classes=1 << 12))),
        (ENUM, (dict(loss_mode=2), dict(loss_mode=-1))),
        (NULL, (dict(logits=None), dict(target=None), dict(loss=None), dict(g_logits=None))),
        (ALIGN, (dict(logits=FAKE + 2), dict(loss=FAKE + 1), dict(g_logits=FAKE + 2), dict(target=FAKE + 4),
                 dict(loss_mode=L.NLL_REGRESSION, target=FAKE + 2))),
    ])
    assert fn(C.byref(_loss(batch=0, loss_mode=9, logits=None)), None) == SHAPE
    assert fn(C.byref(_loss(loss_mode=9, logits=None, loss=FAKE + 1)), None) == ENUM
    assert fn(C.byref(_loss(logits=None, loss=FAKE + 1)), None) == NULL
    assert fn(C.byref(_loss(loss_mode=L.NLL_REGRESSION, target=FAKE + 4, loss=FAKE + 1)), None) == ALIGN   # (4 bytes do for fp32)


def test_ens_bwd_argument_errors():
    L = _L()
    fn = L.load().bnn_ens_bwd
    _refused(fn, _bwd, C.sizeof(L.EnsBwdArgs), [
        (SHAPE, (dict(members=0), dict(first=-1), dict(batch=0), dict(in_features=0), dict(out_features=-2), dict(w_stride=-1),
                 dict(g_stride=-1), dict(batch=1 << 20, in_features=1 << 12), dict(in_features=1 << 16, out_features=1 << 16),
                 dict(members=1 << 20, in_features=1 << 12, out_features=1 << 12))),
        (ENUM, (dict(math=3), dict(math=-1))),
        (NULL, (dict(x=None), dict(gy=None), dict(w=None), dict(g_w=None))),
        (ALIGN, (dict(x=FAKE + 2), dict(gy=FAKE + 1), dict(y=FAKE + 2), dict(w=FAKE + 3), dict(g_w=FAKE + 2), dict(g_b=FAKE + 1),
                 dict(g_x=FAKE + 2))),
    ])
    assert fn(C.byref(_bwd(batch=0, math=9, x=None)), None) == SHAPE
    assert fn(C.byref(_bwd(math=9, x=None, gy=FAKE + 1)), None) == ENUM
    assert fn(C.byref(_bwd(x=None, gy=FAKE + 1)), None) == NULL
    assert fn(C.byref(_bwd(y=None, g_b=None, g_x=None, gy=FAKE + 1)), None) == ALIGN      # (the optional pointers)


def test_host_side_refusals_on_cpu_tensors():
    import networks
    from bnn_hip import ops
    from bnn_hip.ops import BnnHipError
    mp = dict(input_shape=5, classes=3, batch_size=4, hidden_units=6, mode="classification")
    with pytest.raises(BnnHipError):                              # CPU parameters: no fallback
        networks.MLP(mp).ensemble(3)
    with pytest.raises(BnnHipError):
        ops.ens_fwd(torch.zeros(4, 5), torch.zeros(2, 64), 0, None, out_features=3, members=2)
    with pytest.raises(BnnHipError):
        ops.ens_loss(torch.zeros(2, 4, 3), torch.zeros(4, dtype=torch.int64), "classification")
    with pytest.raises(BnnHipError):
        ops.ens_bwd(torch.zeros(4, 5), torch.zeros(2, 4, 3), torch.zeros(2, 64), 0, torch.zeros(2, 64))


# ---------------------------------------------------------------------------------------------- layout and seeds
def test_gradient_bucket_views_follow_bank_layout():
    """Member j's gradient of tensor t is bucket[j, off_t : off_t + numel_t]: the same (offsets, stride) as the bank's
    members, every tensor 256-byte aligned, and a flat [M * stride] view covers members and padding alike."""
    from bnn_hip import ops
    numels = [70 * 37, 70, 65 * 70, 65, 10 * 65, 10]
    offs, stride = ops.bank_layout(numels)
    # every tensor rounded up to 64 elements: 2590 -> 2624, 70 -> 128, 4550 -> 4608, 65 -> 128, 650 -> 704, 10 -> 64
    assert offs == (0, 2624, 2752, 7360, 7488, 8192) and stride == 8256
    M = 3
    bucket = torch.zeros(M, stride)
    flat = bucket.view(-1)
    for j in range(M):
        for t, (o, n) in enumerate(zip(offs, numels)):
            bucket[j, o:o + n] = 100 * j + t + 1
    for j in range(M):
        for t, (o, n) in enumerate(zip(offs, numels)):
            seg = flat[j * stride + o: j * stride + o + n]
            assert seg.data_ptr() == bucket[j, o:].data_ptr() and (seg == 100 * j + t + 1).all()
    covered = sum(numels)
    assert int((flat != 0).sum()) == M * covered and int((flat == 0).sum()) == M * (stride - covered)     # the padding


@pytest.mark.parametrize("cls", ["MLP", "MLP_Dropout"])
def test_seeded_copy_is_reset_parameters_under_the_seed(cls):
    import networks
    from bnn_hip.ensemble import seeded_copy
    mp = dict(input_shape=5, classes=3, batch_size=4, hidden_units=6, mode="regression")
    mlp = getattr(networks, cls)(mp)
    before = {k: v.clone() for k, v in mlp.state_dict().items()}
    torch.manual_seed(99)
    expect_next = torch.rand(4)
    torch.manual_seed(99)
    a, b, c = seeded_copy(mlp, 7), seeded_copy(mlp, 7), seeded_copy(mlp, 8)
    assert torch.equal(torch.rand(4), expect_next)                              # the caller's generator is untouched
    for k, v in mlp.state_dict().items():
        assert torch.equal(v, before[k])                                        # and so is the network
    sa, sb, sc = a.state_dict(), b.state_dict(), c.state_dict()
    assert list(sa) == list(before)
    for k in sa:
        assert torch.equal(sa[k], sb[k]) and not torch.equal(sa[k], sc[k]) and not torch.equal(sa[k], before[k])
    # reset_parameters() of every Linear in layer order under the same seed
    ref = getattr(networks, cls)(mp)
    torch.manual_seed(7)
    for m in ref.net:
        if isinstance(m, torch.nn.Linear):
            m.reset_parameters()
    for k, v in ref.state_dict().items():
        assert torch.equal(v, sa[k])
