"""MC dropout of MLP_Dropout (bnn_dense_fwd / bnn_dense_plan / bnn_dropout_mask, bnn_hip.mcdropout) without a device:
the C ABI's symbols, struct layout, argument checks and launch plan, the Python layer's refusals, and a numpy
restatement of the kind-3 dropout map (include/bnn_hip.h) with its statistics.  tests/test_gpu_mc_dropout.py checks the
kernels against the same restatement."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch
from torch import nn

from oracle.bnn_oracle import philox4x32

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "bnn_hip.h")
NEW_SYMBOLS = {"bnn_dense_fwd", "bnn_dense_plan", "bnn_dropout_mask"}


def dropout_thr_scale(p):
    """thr = min(floor(p 2^32), 2^32 - 1), scale = fp32(1 / (1 - p)), both from fp64."""
    return min(math.floor(p * 2.0 ** 32), 2 ** 32 - 1), np.float32(1.0 / (1.0 - p))


def dropout_mask_np(seed, layer_id, sample, rows, cols, p):
    """The kind-3 map restated: float32 [rows, cols], scale where kept, 0 where dropped."""
    thr, scale = dropout_thr_scale(p)
    gpr = (cols + 3) // 4
    r = np.arange(rows, dtype=np.uint64)[:, None]
    c = np.arange(cols, dtype=np.uint64)[None, :]
    group = ((r * gpr + (c >> np.uint64(2))) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    words = philox4x32(group, np.uint32(sample & 0xFFFFFFFF), np.uint32(4 * layer_id + 3), np.uint32(0),
                       seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    lane = np.broadcast_to((c & np.uint64(3)).astype(np.int64), group.shape)
    w = np.choose(lane, words)
    return np.where(w >= np.uint32(thr), scale, np.float32(0)).astype(np.float32)


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


def test_dense_args_layout_matches_the_header(tmp_path):
    L, _ = _lib()
    cls, cname = L.DenseFwdArgs, "bnn_dense_fwd_args"
    lines = ['printf("%%zu\\n", sizeof(%s));' % cname]
    want = [C.sizeof(cls)]
    for fname, _t in cls._fields_:
        lines.append('printf("%%zu\\n", offsetof(%s, %s));' % (cname, fname))
        want.append(getattr(cls, fname).offset)
    prog = tmp_path / "sz.c"
    prog.write_text('#include "%s"\n#include <stdio.h>\n#include <stddef.h>\nint main(){%s return 0;}' % (HEADER, "".join(lines)))
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", str(prog), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == want


def _args(L, **kw):
    a = L.DenseFwdArgs()
    a.struct_bytes = C.sizeof(L.DenseFwdArgs)
    a.n_samples, a.batch, a.in_features, a.out_features = 10, 128, 784, 1200
    a.x_shared, a.math, a.x_dtype, a.y_dtype = 1, L.MATH_BF16, L.F32, L.BF16
    a.relu, a.layer_id, a.drop_p = 1, 0, 0.5
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_dense_fwd_argument_validation_without_a_device():
    """Every check returns before a launch: nothing here touches a device."""
    L, lib = _lib()
    fake = 0x10000                                     # aligned, never dereferenced: the checks fail first
    a = _args(L)
    a.struct_bytes -= 8
    assert lib.bnn_dense_fwd(C.byref(a), None) == -5
    assert lib.bnn_dense_plan(C.byref(a), C.byref(L.Plan())) == -5
    assert lib.bnn_dense_fwd(None, None) == -1
    for f in ("n_samples", "batch", "in_features", "out_features"):
        for v in (0, -3):
            assert lib.bnn_dense_fwd(C.byref(_args(L, **{f: v}, x=fake, w=fake, y=fake)), None) == -2, (f, v)
    for p in (1.0, 1.5, -0.1, float("nan"), float("inf")):
        assert lib.bnn_dense_fwd(C.byref(_args(L, drop_p=p, x=fake, w=fake, y=fake)), None) == -2, p
    assert lib.bnn_dense_fwd(C.byref(_args(L, layer_id=-1, x=fake, w=fake, y=fake)), None) == -2
    # the counter may only be advanced by a launch that draws no mask
    assert lib.bnn_dense_fwd(C.byref(_args(L, sample_counter_inc=10, sample_counter=fake, x=fake, w=fake, y=fake)), None) == -2
    assert lib.bnn_dense_fwd(C.byref(_args(L, drop_p=0.0, sample_counter_inc=10, x=fake, w=fake, y=fake)), None) == -1
    assert lib.bnn_dense_fwd(C.byref(_args(L, math=7, x=fake, w=fake, y=fake)), None) == -3
    assert lib.bnn_dense_fwd(C.byref(_args(L, math=L.MATH_F32, x=fake, w=fake, y=fake)), None) == -3   # f32 math: fp32 y
    assert lib.bnn_dense_fwd(C.byref(_args(L, x_dtype=5, x=fake, w=fake, y=fake)), None) == -3
    assert lib.bnn_dense_fwd(C.byref(_args(L)), None) == -1                                     # NULL x, w, y
    assert lib.bnn_dense_fwd(C.byref(_args(L, x=fake, y=fake)), None) == -1                     # NULL w
    assert lib.bnn_dense_fwd(C.byref(_args(L, x=fake + 2, w=fake, y=fake)), None) == -6         # fp32 x misaligned
    assert lib.bnn_dense_plan(C.byref(_args(L)), None) == -1


def test_dropout_mask_argument_validation_without_a_device():
    L, lib = _lib()
    fake = 0x10000
    assert lib.bnn_dropout_mask(None, 1, 0, 0, 1, 4, 4, 0.5, None) == -1
    for p in (1.0, 2.0, -1e-9, float("nan")):
        assert lib.bnn_dropout_mask(fake, 1, 0, 0, 1, 4, 4, p, None) == -2, p
    for s, r, c in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4)):
        assert lib.bnn_dropout_mask(fake, 1, 0, 0, s, r, c, 0.5, None) == -2
    assert lib.bnn_dropout_mask(fake + 2, 1, 0, 0, 1, 4, 4, 0.5, None) == -6


def _plan(L, lib, **kw):
    pl = L.Plan()
    assert lib.bnn_dense_plan(C.byref(_args(L, **kw)), C.byref(pl)) == 0
    return {k: getattr(pl, k) for k, _ in L.Plan._fields_}


def test_dense_plan_is_a_pure_function_of_the_shape():
    L, lib = _lib()
    first = _plan(L, lib)
    assert first == _plan(L, lib) == _plan(L, lib, x=0x20000, w=0x40000, y=0x80000, seed=99, sample_offset=7)
    # layer 1 of the reference's evaluation: 2 x 19 tiles of 64 x 64, the 10 samples in 3 runs of <= 4
    assert first["form"] == L.FORM_GEMM and first["batch_rows"] == 64 and first["features_per_block"] == 64
    assert first["k_slices"] == 3 and first["blocks"] == 2 * 19 * 3
    # layer 2: 1280 stacked rows -> 20 x 19 tiles of 64, one pass
    p2 = _plan(L, lib, x_shared=0, in_features=1200, x_dtype=L.BF16)
    assert (p2["batch_rows"], p2["k_slices"], p2["blocks"]) == (64, 1, 20 * 19)
    # the 10 000-row test set at 10 samples: 100 000 rows take the 128 x 128 tile
    p3 = _plan(L, lib, x_shared=0, batch=10000, in_features=1200, x_dtype=L.BF16)
    assert (p3["batch_rows"], p3["features_per_block"], p3["blocks"]) == (128, 128, 782 * 10)
    # exact fp32 always takes the 64 x 64 tile
    p4 = _plan(L, lib, x_shared=0, batch=10000, in_features=1200, math=L.MATH_F32, y_dtype=L.F32)
    assert p4["batch_rows"] == 64 and p4["blocks"] == 1563 * 19
    # many samples of a shared x: no more runs than fill the device, every run non-empty
    p5 = _plan(L, lib, n_samples=256)
    assert p5["k_slices"] == 14 and p5["blocks"] == 38 * 14
    for S in (1, 2, 5, 9, 63):
        pl = _plan(L, lib, n_samples=S)
        per = -(-S // pl["k_slices"])
        assert (pl["k_slices"] - 1) * per < S


def test_dropout_params_and_python_refusals():
    from bnn_hip import BnnHipError, ops
    assert ops.dropout_params(0.5) == (2 ** 31, 2.0)
    assert ops.dropout_params(0.0) == (0, 1.0)
    thr, scale = ops.dropout_params(0.9)
    assert thr == math.floor(0.9 * 2 ** 32) and scale == np.float32(1 / (1 - 0.9))
    for p in (1.0, -0.5, float("nan")):
        with pytest.raises(BnnHipError):
            ops.dropout_params(p)


def _mlp(mode="classification", **kw):
    import networks
    params = dict(input_shape=784 if mode == "classification" else 1, classes=10 if mode == "classification" else 1,
                  batch_size=128, hidden_units=32, mode=mode)
    params.update(kw)
    return networks.MLP_Dropout(params)


def test_mlp_dropout_refusals_without_a_device():
    from bnn_hip import BnnHipError
    mlp = _mlp()
    x = torch.zeros(2, 1, 28, 28)
    with pytest.raises(BnnHipError):                  # CPU parameters / input: no fallback
        mlp.mc_forward(x, 4)
    with pytest.raises(BnnHipError):
        mlp.predict_mc(x, 4)
    with pytest.raises(BnnHipError):                  # quantiles are a regression summary
        mlp.predictive(x, 4, quantiles=(0.5,))
    bad = _mlp()
    bad.net[2] = nn.Dropout(1.0)                      # p outside [0, 1)
    with pytest.raises(BnnHipError):
        bad.mc_forward(x, 4)
    for net in (nn.Sequential(nn.Linear(784, 8), nn.Tanh(), nn.Linear(8, 10)),
                nn.Sequential(nn.Linear(784, 8), nn.ReLU(), nn.Dropout(0.5)),
                nn.Sequential(nn.Linear(784, 8), nn.Dropout(0.5), nn.ReLU(), nn.Linear(8, 10)),
                nn.Sequential(nn.Linear(784, 8), nn.ReLU(), nn.AlphaDropout(0.5), nn.Linear(8, 10))):
        other = _mlp()
        other.net = net
        with pytest.raises(BnnHipError):
            other.mc_forward(x, 4)
    reg = _mlp("regression")
    with pytest.raises(BnnHipError):
        reg.predictive(torch.zeros(3, 1), 4, quantiles=(0.1, 2.0))


SEED = 0x0123456789ABCDEF


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_restated_keep_rate(p):
    rows, cols = 257, 1003
    n = rows * cols
    kept = sum(int(np.count_nonzero(dropout_mask_np(SEED, layer, s, rows, cols, p))) for layer, s in ((0, 0), (1, 5)))
    n *= 2
    sd = math.sqrt(n * p * (1 - p))
    assert abs(kept - n * (1 - p)) < 5 * sd
    m = dropout_mask_np(SEED, 0, 3, rows, cols, p)
    assert set(np.unique(m).tolist()) == {0.0, float(np.float32(1 / (1 - p)))}


def test_restated_p0_keeps_everything():
    m = dropout_mask_np(SEED, 2, 11, 64, 37, 0.0)
    assert np.all(m == 1.0)


def test_restated_masks_are_uncorrelated():
    """Keep indicators of different layers, samples, neighbouring rows and neighbouring columns are uncorrelated."""
    rows, cols, p = 512, 512, 0.5
    a = dropout_mask_np(SEED, 0, 0, rows, cols, p) > 0
    pairs = {
        "layer": (a, dropout_mask_np(SEED, 1, 0, rows, cols, p) > 0),
        "sample": (a, dropout_mask_np(SEED, 0, 1, rows, cols, p) > 0),
        "row": (a[:-1], a[1:]),
        "col": (a[:, :-1], a[:, 1:]),
        "col+4": (a[:, :-4], a[:, 4:]),
        "seed": (a, dropout_mask_np(SEED + 1, 0, 0, rows, cols, p) > 0),
    }
    for name, (u, v) in pairs.items():
        u, v = u.ravel().astype(np.float64), v.ravel().astype(np.float64)
        r = np.corrcoef(u, v)[0, 1]
        assert abs(r) < 5 / math.sqrt(u.size), (name, r)
