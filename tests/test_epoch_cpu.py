"""CPU-side checks of the device epoch loader (bnn_epoch_permutation / bnn_epoch_stage, bnn_hip.epoch, bnn_hip.tasks; no
GPU): the entry points exist, the ctypes mirrors match the header, every argument check runs on the host before a launch,
the CPU restatement of the permutation (tests/epoch_ref.py) is a permutation built on the oracle's Philox, the host beta
table is the golden schedule, the loader's length and drop_last rule, and the wrappers' reference surface."""
import ctypes as C

import numpy as np
import pytest
import torch

import epoch_ref as R
from oracle import bnn_oracle as O
from test_bandit_cpu import _layout

FAKE = 0x10000
SIZES = (1, 5, 128, 8192, 8193, 60000)


def test_epoch_exports_and_abi_version():
    from bnn_hip import _lib as L
    lib = L.load()
    assert lib.bnn_version() == 9 == L.ABI_VERSION
    for name in ("bnn_epoch_permutation", "bnn_epoch_stage"):
        assert name in L.EXPORTS and hasattr(lib, name)


def test_epoch_struct_layouts_match_the_header(tmp_path):
    from bnn_hip import _lib as L
    _layout(tmp_path, L.EpochPermArgs, "bnn_epoch_perm_args",
            [("BNN_EPOCH_MAX_ROWS", L.EPOCH_MAX_ROWS), ("BNN_EPOCH_MAX_LOSS_COLS", L.EPOCH_MAX_LOSS_COLS),
             ("BNN_EPOCH_X_F32", L.EPOCH_X_F32), ("BNN_EPOCH_X_U8", L.EPOCH_X_U8), ("BNN_HIP_ABI_VERSION", L.ABI_VERSION)])
    _layout(tmp_path, L.EpochStageArgs, "bnn_epoch_stage_args")
    assert L.EPOCH_MAX_ROWS >= 65536


def _perm_args(**over):
    from bnn_hip import _lib as L
    a = L.EpochPermArgs()
    a.struct_bytes = C.sizeof(L.EpochPermArgs)
    a.n_rows, a.seed, a.epoch, a.order = 100, 7, FAKE, FAKE
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _stage_args(**over):
    from bnn_hip import _lib as L
    a = L.EpochStageArgs()
    a.struct_bytes = C.sizeof(L.EpochStageArgs)
    a.n_rows, a.row_dim, a.batch_size, a.num_batches, a.x_dtype, a.target_dim = 100, 12, 8, 12, L.EPOCH_X_F32, 0
    for f in ("x", "targets", "batch_index", "epoch", "ticket", "x_out", "targets_out"):
        setattr(a, f, FAKE)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_permutation_argument_validation_without_a_device():
    """Fake, never dereferenced device addresses: every rejection happens before a launch."""
    from bnn_hip import _lib as L
    fn = L.load().bnn_epoch_permutation
    assert fn(None, None) == -1                                                           # BNN_ERR_NULL
    assert fn(C.byref(_perm_args(struct_bytes=C.sizeof(L.EpochPermArgs) + 8)), None) == -5   # BNN_ERR_ABI
    for bad in (dict(n_rows=0), dict(n_rows=-3), dict(n_rows=L.EPOCH_MAX_ROWS + 1)):
        assert fn(C.byref(_perm_args(**bad)), None) == -2, bad                            # BNN_ERR_SHAPE
    for f in ("epoch", "order"):
        assert fn(C.byref(_perm_args(**{f: None})), None) == -1, f
    assert fn(C.byref(_perm_args(order=FAKE + 2)), None) == -6                            # BNN_ERR_ALIGN


def test_stage_argument_validation_without_a_device():
    from bnn_hip import _lib as L
    fn = L.load().bnn_epoch_stage
    assert fn(None, None) == -1
    assert fn(C.byref(_stage_args(struct_bytes=C.sizeof(L.EpochStageArgs) - 8)), None) == -5
    for bad in (dict(n_rows=L.EPOCH_MAX_ROWS + 1), dict(n_rows=0), dict(num_batches=13), dict(batch_size=9), dict(batch_size=0),
                dict(num_batches=0), dict(row_dim=0), dict(target_dim=-1), dict(loss_cols=5), dict(loss_history=FAKE)):
        assert fn(C.byref(_stage_args(**bad)), None) == -2, bad                           # B M > N and the other shapes
    for code in (2, -1, 7):
        assert fn(C.byref(_stage_args(x_dtype=code)), None) == -3, code                   # BNN_ERR_ENUM
    for f in ("x", "targets", "batch_index", "epoch", "ticket", "x_out", "targets_out"):
        assert fn(C.byref(_stage_args(**{f: None})), None) == -1, f
    assert fn(C.byref(_stage_args(beta_table=FAKE)), None) == -1                          # a table without its word
    assert fn(C.byref(_stage_args(loss_history=FAKE, loss_cols=2)), None) == -1           # a history without its sources
    assert fn(C.byref(_stage_args(x_out=FAKE + 2)), None) == -6
    assert fn(C.byref(_stage_args(targets_out=FAKE + 4)), None) == -6                     # int64 labels


@pytest.mark.parametrize("N", SIZES)
def test_reference_permutation_is_a_permutation(N):
    p = R.permutation(0x5EED0123456789AB, 3, N)
    assert p.dtype == np.int32 and np.array_equal(np.sort(p), np.arange(N))


def test_reference_permutation_differs_between_epochs_and_seeds():
    a, b, c = R.permutation(11, 0, 8193), R.permutation(11, 1, 8193), R.permutation(12, 0, 8193)
    assert not np.array_equal(a, b) and not np.array_equal(a, c) and not np.array_equal(b, c)
    assert np.array_equal(a, R.permutation(11, 0, 8193))


def test_reference_keys_are_the_oracle_philox_words():
    """key_p = word (p & 3) of the oracle's Philox4x32 at counter (p >> 2, epoch, 2, 1): word 3 = 1 keeps the stream off
    every eps counter, word 2 = 2 off the bandit's two streams ((.., 0, 1) and (.., 1, 1))."""
    seed, epoch, N = 0x123456789ABCDEF0, 5, 37
    assert R.COUNTER_WORDS == (2, 1)
    k = R.keys(seed, epoch, N)
    for p in (0, 1, 2, 3, 4, 17, 36):
        w = O.philox4x32(p >> 2, epoch, 2, 1, seed & 0xFFFFFFFF, seed >> 32)
        assert int(k[p]) == int(np.asarray(w[p & 3]).reshape(()))
    order = R.permutation(seed, epoch, N)
    pairs = [(int(k[p]), int(p)) for p in order]
    assert pairs == sorted(pairs)


def test_host_beta_table_equals_the_golden_schedule(g_beta):
    from bnn_hip import epoch
    c = g_beta.case("G9")
    M = int(c["M"])
    t = epoch.beta_table(M)
    assert t.dtype == np.float32 and t.shape == (M,)
    for i, idx in enumerate(c["idx"]):
        assert t[int(idx)] == np.float32(c["beta"][i]) == R.beta(M, int(idx))
    for M in (1, 8, 468):
        t = epoch.beta_table(M)
        assert [float(v) for v in t] == [float(np.float32(O.beta_schedule(M, j))) for j in range(M)]


def test_loader_length_and_drop_last_rule():
    from bnn_hip import epoch
    from bnn_hip.ops import BnnHipError
    ds = epoch.DeviceDataset(np.zeros((1000, 1, 4, 4), np.uint8), np.zeros(1000, np.int64), device="cpu")
    assert len(ds) == 1000 and tuple(ds.x.shape) == (1000, 16) and ds.item_shape == (1, 4, 4)
    assert len(epoch.DeviceLoader(ds, 128)) == 7 and len(epoch.DeviceLoader(ds, 128, shuffle=False)) == 7
    assert len(epoch.DeviceLoader(ds, 125, drop_last=False)) == 8
    with pytest.raises(BnnHipError, match="drop_last"):
        epoch.DeviceLoader(ds, 128, drop_last=False)
    with pytest.raises(BnnHipError, match="batch_size"):
        epoch.DeviceLoader(ds, 1001)
    reg = epoch.DeviceDataset(np.zeros((1024, 1), np.float32), np.zeros((1024, 1), np.float32), device="cpu")
    assert len(epoch.DeviceLoader(reg, 128, drop_last=False)) == 8 and tuple(reg.y.shape) == (1024, 1)
    with pytest.raises(BnnHipError, match="uint8 or float32"):
        epoch.DeviceDataset(np.zeros((8, 2), np.float64), np.zeros(8, np.int64), device="cpu")
    with pytest.raises(BnnHipError, match="rows"):
        epoch.DeviceDataset(np.zeros((65537, 1), np.uint8), np.zeros(65537, np.int64), device="cpu")
    with pytest.raises(BnnHipError, match="no CPU fallback"):                              # nothing runs off the device
        next(iter(epoch.DeviceLoader(ds, 128)))


# the reference's surface (classification/class_task.py, regression/reg_task.py), by name
CLASS_METHODS = ("init_net", "train_step", "predict", "evaluate", "log_progress")
REG_METHODS = ("init_net", "train_step", "evaluate", "log_progress")
SURFACE = {
    "BNN_Classification": (CLASS_METHODS, ("label", "lr", "hidden_units", "mode", "batch_size", "num_batches", "n_samples", "test_samples",
                                           "x_shape", "classes", "mu_init", "rho_init", "prior_init", "mixture_prior", "save_model_path",
                                           "local_reparam", "best_acc", "net", "optimiser", "scheduler", "writer")),
    "MLP_Classification": (CLASS_METHODS, ("label", "lr", "hidden_units", "mode", "batch_size", "num_batches", "x_shape", "classes",
                                           "save_model_path", "best_acc", "dropout", "net", "optimiser", "scheduler", "writer")),
    "MCDropout_Classification": (CLASS_METHODS, ("label", "lr", "hidden_units", "mode", "batch_size", "num_batches", "test_samples",
                                                 "x_shape", "classes", "save_model_path", "best_acc", "dropout", "net", "optimiser",
                                                 "scheduler", "writer")),
    "BNN_Regression": (REG_METHODS, ("label", "batch_size", "num_batches", "n_samples", "test_samples", "x_shape", "y_shape", "noise_tol",
                                     "lr", "save_model_path", "local_reparam", "best_loss", "net", "optimiser", "scheduler", "writer")),
    "MLP_Regression": (REG_METHODS, ("label", "lr", "hidden_units", "mode", "batch_size", "num_batches", "x_shape", "y_shape",
                                     "save_model_path", "best_loss", "net", "optimiser", "scheduler", "writer")),
    "MCDropout_Regression": (REG_METHODS, ("label", "lr", "hidden_units", "mode", "batch_size", "num_batches", "test_samples", "x_shape",
                                           "y_shape", "save_model_path", "best_loss", "net", "optimiser", "scheduler", "writer")),
}


@pytest.mark.parametrize("name", sorted(SURFACE))
def test_wrappers_expose_the_reference_surface(name, tmp_path, monkeypatch):
    import config
    import networks
    from bnn_hip import tasks
    from bnn_hip.optim import FusedAdam, FusedSGD
    monkeypatch.setattr(config, "DEVICE", torch.device("cpu"))         # construction only: nothing is launched
    klass = name.endswith("Classification")
    params = dict(lr=1e-3, hidden_units=8, mode="classification" if klass else "regression", batch_size=4, num_batches=3,
                  train_samples=2, test_samples=3, x_shape=16 if klass else 1, classes=3, y_shape=1, noise_tolerance=0.1,
                  mu_init=[-0.2, 0.2], rho_init=[-5, -4], prior_init=[1.0], mixture_prior=False, local_reparam=False,
                  dropout=True, save_dir=str(tmp_path / "saved"), epochs=1)
    methods, attrs = SURFACE[name]
    t = getattr(tasks, name)(name.lower(), params)
    for m in methods:
        assert callable(getattr(t, m)), m
    for a in attrs:
        assert hasattr(t, a), a
    assert (tmp_path / "saved").is_dir() and t.save_model_path.endswith(f"{name.lower()}_model.pt")
    assert isinstance(t.scheduler, torch.optim.lr_scheduler.StepLR)
    want_net = {"BNN": networks.BayesianNetwork, "MLP": networks.MLP, "MCDropout": networks.MLP_Dropout}[name.split("_")[0]]
    if name == "MLP_Classification":
        want_net = networks.MLP_Dropout                                 # dropout=True above
    assert type(t.net) is want_net
    assert isinstance(t.optimiser, FusedSGD if name in ("MLP_Classification", "MCDropout_Classification") else FusedAdam)
    assert (t.best_acc == 0.0) if klass else (t.best_loss == np.inf)
    t.log_progress(0)                                                   # no writer: a no-op
