"""Training MLP / MLP_Dropout on the device (bnn_dense_loss / bnn_dense_bwd / bnn_sgd_step, bnn_hip.optim.FusedSGD,
bnn_hip.dense_train.GraphedDenseTrainStep) without a device: the C ABI's symbols, struct layouts and argument checks,
the Python layer's refusals, and a numpy restatement of the loss kernel's definition.  tests/test_gpu_dense_train.py
runs the kernels against fp64 restatements and PyTorch."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch
from torch import nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "bnn_hip.h")
NEW_SYMBOLS = {"bnn_dense_loss", "bnn_dense_bwd", "bnn_sgd_step"}
FAKE = 0x10000                      # aligned, never dereferenced: the checks fail first


def dense_loss_np(z, target, mode, grad_scale=1.0):
    """The loss kernel's definition in fp64: (loss, g_logits).  cross_entropy(sum): sum_b logsumexp(z_b) - z_b[y_b],
    gradient softmax(z) - onehot(y); an out-of-range label makes the loss and its row NaN.  mse_loss(sum): sum (z - y)^2,
    gradient 2 (z - y).  Both gradients times grad_scale."""
    z = np.asarray(z, dtype=np.float64)
    if mode == "classification":
        B, Cc = z.shape
        mx = z.max(axis=1, keepdims=True)
        e = np.exp(z - mx)
        lse = mx[:, 0] + np.log(e.sum(axis=1))
        ok = (target >= 0) & (target < Cc)
        picked = np.where(ok, z[np.arange(B), np.where(ok, target, 0)], np.nan)
        rows = np.where(ok, lse - picked, np.nan)
        g = e / e.sum(axis=1, keepdims=True)
        g[np.arange(B)[ok], target[ok]] -= 1.0
        g[~ok] = np.nan
        return rows.sum(), g * grad_scale
    d = z - np.asarray(target, dtype=np.float64).reshape(z.shape)
    return (d * d).sum(), 2.0 * d * grad_scale


def _lib():
    from bnn_hip import _lib
    return _lib, _lib.load()


def test_new_symbols_are_exported_and_declared():
    import re
    L, lib = _lib()
    declared = set(re.findall(r"\b(bnn_[a-z0-9_]+)\s*\(", open(HEADER).read()))
    assert NEW_SYMBOLS <= declared
    assert NEW_SYMBOLS <= set(L.EXPORTS)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
    assert L.ABI_VERSION == 9 and lib.bnn_version() == 9


def test_new_struct_layouts_match_the_header(tmp_path):
    L, _ = _lib()
    lines, want = [], []
    for cname, cls in (("bnn_dense_loss_args", L.DenseLossArgs), ("bnn_dense_bwd_args", L.DenseBwdArgs),
                       ("bnn_sgd_args", L.SgdArgs)):
        lines.append('printf("%%zu\\n", sizeof(%s));' % cname)
        want.append(C.sizeof(cls))
        for fname, _t in cls._fields_:
            lines.append('printf("%%zu\\n", offsetof(%s, %s));' % (cname, fname))
            want.append(getattr(cls, fname).offset)
    prog = tmp_path / "sz.c"
    prog.write_text('#include "%s"\n#include <stdio.h>\n#include <stddef.h>\nint main(){%s return 0;}' % (HEADER, "".join(lines)))
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", str(prog), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == want
    assert L.SGD_MAX_TENSORS == 16 and "#define BNN_SGD_MAX_TENSORS 16" in open(HEADER).read()


def _loss_args(L, **kw):
    a = L.DenseLossArgs()
    a.struct_bytes = C.sizeof(L.DenseLossArgs)
    a.batch, a.classes, a.loss_mode, a.grad_scale = 128, 10, L.NLL_CLASSIFICATION, 1.0
    a.logits, a.target, a.loss, a.g_logits = FAKE, FAKE, FAKE, FAKE
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_dense_loss_argument_validation_without_a_device():
    L, lib = _lib()
    assert lib.bnn_dense_loss(None, None) == -1
    a = _loss_args(L)
    a.struct_bytes -= 4
    assert lib.bnn_dense_loss(C.byref(a), None) == -5
    for f in ("batch", "classes"):
        for v in (0, -1):
            assert lib.bnn_dense_loss(C.byref(_loss_args(L, **{f: v})), None) == -2, (f, v)
    assert lib.bnn_dense_loss(C.byref(_loss_args(L, loss_mode=2)), None) == -3
    for f in ("logits", "target", "loss", "g_logits"):
        assert lib.bnn_dense_loss(C.byref(_loss_args(L, **{f: None})), None) == -1, f
    assert lib.bnn_dense_loss(C.byref(_loss_args(L, logits=FAKE + 2)), None) == -6
    assert lib.bnn_dense_loss(C.byref(_loss_args(L, target=FAKE + 4)), None) == -6                   # int64 labels


def _bwd_args(L, **kw):
    a = L.DenseBwdArgs()
    a.struct_bytes = C.sizeof(L.DenseBwdArgs)
    a.batch, a.in_features, a.out_features, a.math = 128, 784, 1200, L.MATH_F32
    a.x, a.gy, a.w, a.g_w = FAKE, FAKE, FAKE, FAKE
    a.y_scale, a.gx_scale = 2.0, 2.0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_dense_bwd_argument_validation_without_a_device():
    L, lib = _lib()
    assert lib.bnn_dense_bwd(None, None) == -1
    a = _bwd_args(L)
    a.struct_bytes += 8
    assert lib.bnn_dense_bwd(C.byref(a), None) == -5
    for f in ("batch", "in_features", "out_features"):
        for v in (0, -7):
            assert lib.bnn_dense_bwd(C.byref(_bwd_args(L, **{f: v})), None) == -2, (f, v)
    assert lib.bnn_dense_bwd(C.byref(_bwd_args(L, batch=1 << 20, in_features=1 << 12)), None) == -2
    assert lib.bnn_dense_bwd(C.byref(_bwd_args(L, math=9)), None) == -3
    for f in ("x", "gy", "w", "g_w"):
        assert lib.bnn_dense_bwd(C.byref(_bwd_args(L, **{f: None})), None) == -1, f
    for f in ("x", "gy", "y", "w", "g_w", "g_b", "g_x"):
        assert lib.bnn_dense_bwd(C.byref(_bwd_args(L, **{f: FAKE + 1})), None) == -6, f


def _sgd_args(L, n=2, **kw):
    a = L.SgdArgs()
    a.struct_bytes = C.sizeof(L.SgdArgs)
    a.n_tensors = n
    for t in range(n):
        a.param[t], a.grad[t], a.numel[t] = FAKE, FAKE, 100
    a.lr = 0.1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_sgd_step_argument_validation_without_a_device():
    L, lib = _lib()
    assert lib.bnn_sgd_step(None, None) == -1
    a = _sgd_args(L)
    a.struct_bytes -= 8
    assert lib.bnn_sgd_step(C.byref(a), None) == -5
    for n in (0, -1, 17):
        assert lib.bnn_sgd_step(C.byref(_sgd_args(L, n=max(0, min(n, 16)), n_tensors=n)), None) == -2, n
    for lr in (-0.1, float("nan")):
        assert lib.bnn_sgd_step(C.byref(_sgd_args(L, lr=lr)), None) == -2
    assert lib.bnn_sgd_step(C.byref(_sgd_args(L, weight_decay=-1.0)), None) == -2
    a = _sgd_args(L)
    a.numel[1] = 0
    assert lib.bnn_sgd_step(C.byref(a), None) == -2
    a = _sgd_args(L)
    a.grad[1] = None
    assert lib.bnn_sgd_step(C.byref(a), None) == -1
    a = _sgd_args(L)
    a.param[0] = FAKE + 4
    assert lib.bnn_sgd_step(C.byref(a), None) == -6
    assert lib.bnn_sgd_step(C.byref(_sgd_args(L, lr_device=FAKE + 2)), None) == -6


def test_dense_loss_restatement():
    """The numpy restatement against torch's own cross_entropy / mse_loss (sum) and autograd, in fp64."""
    rng = np.random.default_rng(3)
    for B, Cc in ((128, 10), (5, 3), (1, 1), (7, 1)):
        z = rng.normal(scale=3.0, size=(B, Cc))
        y = rng.integers(0, Cc, size=B)
        zt = torch.tensor(z, requires_grad=True)
        ref = torch.nn.functional.cross_entropy(zt, torch.tensor(y), reduction="sum")
        ref.backward()
        loss, g = dense_loss_np(z, y, "classification", 0.5)
        np.testing.assert_allclose(loss, ref.item(), rtol=1e-12)
        np.testing.assert_allclose(g, 0.5 * zt.grad.numpy(), rtol=1e-12, atol=1e-15)
        t = rng.normal(size=(B, Cc))
        zt = torch.tensor(z, requires_grad=True)
        ref = torch.nn.functional.mse_loss(zt, torch.tensor(t), reduction="sum")
        ref.backward()
        loss, g = dense_loss_np(z, t, "regression")
        np.testing.assert_allclose(loss, ref.item(), rtol=1e-12)
        np.testing.assert_allclose(g, zt.grad.numpy(), rtol=1e-12)
    # large logits: logsumexp stays finite
    loss, g = dense_loss_np(np.array([[1000.0, 0.0, -1000.0]]), np.array([0]), "classification")
    assert loss == pytest.approx(0.0, abs=1e-12) and np.isfinite(g).all()


def test_dense_loss_restatement_poisons_out_of_range_labels():
    z = np.random.default_rng(0).normal(size=(4, 5))
    for bad in (-1, 5, 1 << 40):
        y = np.array([0, bad, 2, 4])
        loss, g = dense_loss_np(z, y, "classification")
        assert np.isnan(loss)
        assert np.isnan(g[1]).all() and np.isfinite(np.delete(g, 1, axis=0)).all()


def _mlp(cls="MLP_Dropout", mode="classification", hidden=16):
    import networks
    params = dict(input_shape=784 if mode == "classification" else 1, classes=10 if mode == "classification" else 1,
                  batch_size=128, hidden_units=hidden, mode=mode)
    return getattr(networks, cls)(params)


def test_fused_sgd_refusals_and_state_dict_without_a_device():
    from bnn_hip import BnnHipError
    from bnn_hip.optim import FusedSGD
    mlp = _mlp()
    for kw in (dict(momentum=0.9), dict(nesterov=True), dict(maximize=True), dict(dampening=0.1)):
        with pytest.raises(BnnHipError):
            FusedSGD(mlp.parameters(), lr=0.1, **kw)
    with pytest.raises(ValueError):
        FusedSGD(mlp.parameters(), lr=-1.0)
    with pytest.raises(ValueError):
        FusedSGD(mlp.parameters(), lr=0.1, weight_decay=-1.0)
    opt = FusedSGD(mlp.parameters(), lr=0.25, weight_decay=1e-4)
    for p in mlp.parameters():
        p.grad = torch.zeros_like(p)
    with pytest.raises(BnnHipError):              # CPU tensors: no fallback
        opt.step()
    # state dicts interoperate with torch.optim.SGD both ways
    ref = torch.optim.SGD(mlp.parameters(), lr=0.5, weight_decay=1e-3)
    sd = ref.state_dict()
    opt.load_state_dict(sd)
    assert opt.param_groups[0]["lr"] == 0.5 and opt.param_groups[0]["weight_decay"] == 1e-3
    assert opt.param_groups[0]["capturable"] is False
    ours = opt.state_dict()
    for k, v in sd["param_groups"][0].items():
        assert ours["param_groups"][0][k] == v, k
    ref2 = torch.optim.SGD(mlp.parameters(), lr=0.1)
    ref2.load_state_dict(ours)
    assert ref2.param_groups[0]["lr"] == 0.5
    with pytest.raises(BnnHipError):              # a momentum SGD's state is refused, not ignored
        opt.load_state_dict(torch.optim.SGD(mlp.parameters(), lr=0.1, momentum=0.9).state_dict())
    # scheduler: StepLR turns param_groups[i]['lr'] as on torch's SGD
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    opt.param_groups[0]["lr"] = 0.5
    sched.step()
    assert opt.param_groups[0]["lr"] == 0.25


def test_graphed_dense_train_step_refusals_without_a_device():
    from bnn_hip import BnnHipError, runtime
    from bnn_hip.dense_train import GraphedDenseTrainStep
    from bnn_hip.optim import FusedAdam, FusedSGD
    mlp = _mlp()
    x, y = torch.zeros(4, 1, 28, 28), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(BnnHipError):              # a non-capturable optimiser
        mlp.graphed_train_step(FusedSGD(mlp.parameters(), lr=0.1), x, y)
    with pytest.raises(BnnHipError):
        mlp.graphed_train_step(FusedAdam(mlp.parameters(), lr=0.1), x, y)
    with pytest.raises(BnnHipError):              # not one of the fused optimisers
        mlp.graphed_train_step(torch.optim.SGD(mlp.parameters(), lr=0.1), x, y)
    sgd = FusedSGD(mlp.parameters(), lr=0.1, capturable=True)
    sgd.param_groups[0]["momentum"] = 0.9         # momentum turned on after construction
    with pytest.raises(BnnHipError):
        GraphedDenseTrainStep(mlp, sgd, x, y)
    for key in ("nesterov", "maximize"):
        sgd = FusedSGD(mlp.parameters(), lr=0.1, capturable=True)
        sgd.param_groups[0][key] = True
        with pytest.raises(BnnHipError):
            GraphedDenseTrainStep(mlp, sgd, x, y)
    opt = FusedSGD(mlp.parameters(), lr=0.1, capturable=True)
    with pytest.raises(BnnHipError):              # CPU parameters and tensors
        mlp.graphed_train_step(opt, x, y)
    for net in (nn.Sequential(nn.Linear(784, 8), nn.Tanh(), nn.Linear(8, 10)),
                nn.Sequential(nn.Linear(784, 8), nn.ReLU(), nn.Dropout(0.5)),
                nn.Sequential(nn.Linear(784, 8), nn.Dropout(0.5), nn.ReLU(), nn.Linear(8, 10))):
        other = _mlp()
        other.net = net
        with pytest.raises(BnnHipError):
            other.graphed_train_step(FusedSGD(other.parameters(), lr=0.1, capturable=True), x, y)
    half = _mlp("MLP").half()
    with pytest.raises(BnnHipError):              # non-fp32 parameters
        half.graphed_train_step(FusedSGD(half.parameters(), lr=0.1, capturable=True), x.half(), y)
    runtime.shard_samples(True)
    try:
        with pytest.raises(BnnHipError):          # MC-sample sharding on
            mlp.graphed_train_step(opt, x, y)
    finally:
        runtime.shard_samples(False)
    with pytest.raises(BnnHipError):              # unknown loss
        mlp.graphed_train_step(opt, x, y, loss="hinge")
