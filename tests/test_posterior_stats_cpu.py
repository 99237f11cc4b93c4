"""CPU-side checks of F11 (bnn_param_hist, bnn_hip.diagnostics; no GPU): the entry points exist, the ctypes mirrors and
constants match the header, every argument check runs before a launch, the TensorBoard bin table and the trimming rule
equal their restatements (tests/posterior_stats_ref.py), and log_progress writes the reference's tags."""
import ctypes as C

import numpy as np
import pytest
import torch

import posterior_stats_ref as R
from test_bandit_cpu import _layout

FAKE = 0x10000


def test_exports_struct_layouts_and_constants(tmp_path):
    from bnn_hip import _lib as L
    lib = L.load()
    assert lib.bnn_version() == 9 == L.ABI_VERSION
    for name in ("bnn_param_hist", "bnn_param_hist_workspace_bytes"):
        assert name in L.EXPORTS and hasattr(lib, name)
    _layout(tmp_path, L.ParamHistArgs, "bnn_param_hist_args",
            [("BNN_HIST_MAX_JOBS", L.HIST_MAX_JOBS), ("BNN_HIST_MAX_EDGES", L.HIST_MAX_EDGES), ("BNN_HIST_CHUNK", L.HIST_CHUNK),
             ("BNN_HIST_VALUE", L.HIST_VALUE), ("BNN_HIST_SIGMA", L.HIST_SIGMA), ("BNN_HIST_SNR_DB", L.HIST_SNR_DB),
             ("BNN_HIST_SAMPLE", L.HIST_SAMPLE), ("(int)BNN_HIST_RECORD_BYTES(2)", L.hist_record_bytes(2)),
             ("(int)BNN_HIST_RECORD_BYTES(2048)", L.hist_record_bytes(2048)), ("BNN_HIP_ABI_VERSION", L.ABI_VERSION)])
    _layout(tmp_path, L.ParamHistJob, "bnn_param_hist_job")
    _layout(tmp_path, L.HistSummary, "bnn_hist_summary")
    assert L.HIST_MAX_JOBS >= 16 and L.HIST_MAX_EDGES >= 2048


def _args(n_jobs=2, n_edges=3, **over):
    from bnn_hip import _lib as L
    a = L.ParamHistArgs()
    a.struct_bytes = C.sizeof(L.ParamHistArgs)
    a.n_jobs, a.n_edges, a.edges, a.workspace, a.workspace_bytes = n_jobs, n_edges, FAKE, FAKE, 1 << 20
    for i in range(min(n_jobs, L.HIST_MAX_JOBS)):
        j = a.jobs[i]
        j.kind, j.n, j.src0, j.src1, j.record = L.HIST_VALUE, 10, FAKE, FAKE, FAKE
    for k, v in over.items():
        if k.startswith("job_"):
            setattr(a.jobs[1], k[4:], v)
        else:
            setattr(a, k, v)
    return a


def test_c_abi_argument_validation_without_a_device():
    """Fake, never dereferenced device addresses: every rejection happens before a launch."""
    from bnn_hip import _lib as L
    lib = L.load()
    fn, ws = lib.bnn_param_hist, lib.bnn_param_hist_workspace_bytes
    assert fn(None, None) == -1 and ws(None) == 0
    assert fn(C.byref(_args(struct_bytes=8)), None) == -5
    for bad in (dict(n_jobs=0), dict(n_jobs=L.HIST_MAX_JOBS + 1), dict(n_edges=1), dict(n_edges=L.HIST_MAX_EDGES + 1),
                dict(job_n=-1), dict(job_n=1 << 31), dict(job_kind=L.HIST_SAMPLE, job_rows=2, job_cols=4),
                dict(job_kind=L.HIST_SAMPLE, job_rows=0, job_cols=10)):
        assert fn(C.byref(_args(**bad)), None) == -2, bad
        assert ws(C.byref(_args(**bad))) == 0, bad
    for kind in (-1, 4):
        assert fn(C.byref(_args(job_kind=kind)), None) == -3
    for bad in (dict(edges=None), dict(job_src0=None), dict(job_record=None), dict(job_kind=L.HIST_SNR_DB, job_src1=None)):
        assert fn(C.byref(_args(**bad)), None) == -1, bad
    assert fn(C.byref(_args(job_n=0, job_src0=None)), None) != -1                          # an empty job needs no source
    assert fn(C.byref(_args(workspace=None)), None) == -4 and fn(C.byref(_args(workspace_bytes=8)), None) == -4
    for bad in (dict(job_src0=FAKE + 2), dict(job_values_out=FAKE + 1), dict(job_record=FAKE + 4), dict(edges=FAKE + 4),
                dict(workspace=FAKE + 4)):
        assert fn(C.byref(_args(**bad)), None) == -6, bad
    for table in ([0.0, 1.0, 1.0], [0.0, 2.0, 1.0], [0.0, np.nan, 1.0], [0.0, 1.0, np.inf]):      # the optional host copy
        e = np.array(table, np.float64)
        assert fn(C.byref(_args(edges_host=e.ctypes.data)), None) == -2, table
    # the workspace: one 24-byte partial per BNN_HIST_CHUNK elements of a job
    assert ws(C.byref(_args(job_n=3 * L.HIST_CHUNK + 1))) == 24 * (1 + 4)


def test_c_abi_empty_jobs_only_need_no_source():
    from bnn_hip import _lib as L
    a = _args(n_jobs=1)
    a.jobs[0].n, a.jobs[0].src0 = 0, None
    assert L.load().bnn_param_hist_workspace_bytes(C.byref(a)) == 24


def test_tensorboard_bins_equal_the_writer_loop():
    from bnn_hip import diagnostics as D
    buckets, table = R.default_bins()
    e = D.tensorboard_bins()
    assert e.dtype == np.float64 and len(e) == 2 * len(buckets) + 1 == len(table)
    assert all(float(a) == b for a, b in zip(e, table))
    assert e[len(buckets)] == 0.0 and np.all(np.diff(e) > 0) and len(e) <= 2048
    u = D.uniform_bins(-40.0, 20.0, 60)
    assert u.dtype == np.float64 and len(u) == 61 and u[0] == -40.0 and u[-1] == 20.0 and np.all(np.diff(u) > 0)


@pytest.mark.parametrize("case", ["zero", "first", "last", "middle", "both_ends"])
def test_trimming_equals_make_histogram_rule(case):
    from bnn_hip import diagnostics as D
    limits = np.arange(9, dtype=np.float64)
    counts = np.zeros(8, np.int64)
    if case in ("first", "both_ends"):
        counts[0] = 3
    if case in ("last", "both_ends"):
        counts[-1] = 2
    if case == "middle":
        counts[3:5] = (4, 1)
    c, l = D.trim_histogram(counts, limits)
    rc, rl = R.trim(counts, limits)
    if case == "zero":                                       # the rule's slices are empty there (make_histogram raises)
        assert rc.size == 0 and c.size == 0 and l.size == 0
        return
    assert c.tolist() == rc.tolist() and l.tolist() == rl.tolist() and len(c) == len(l)
    want = {"first": ([0, 3], [0.0, 1.0]), "last": ([0, 2], [7.0, 8.0]), "middle": ([0, 4, 1], [3.0, 4.0, 5.0]),
            "both_ends": ([0, 3, 0, 0, 0, 0, 0, 0, 2], list(map(float, range(9))))}[case]
    assert (c.tolist(), l.tolist()) == want


def _cpu_net(local_reparam=False):
    import networks
    return networks.BayesianNetwork({'input_shape': 16, 'classes': 3, 'batch_size': 4, 'hidden_units': 8, 'mode': 'classification',
                                     'mu_init': [-0.2, 0.2], 'rho_init': [-5, -4], 'prior_init': [1.0], 'mixture_prior': False,
                                     'local_reparam': local_reparam})


def test_python_validation_errors():
    from bnn_hip import _lib as L
    from bnn_hip import diagnostics as D
    from bnn_hip import ops
    from bnn_hip.ops import BnnHipError
    t = torch.zeros(8)
    with pytest.raises(BnnHipError, match="strictly increasing"):
        ops.param_hist_args([dict(kind=L.HIST_VALUE, src0=t)], [0.0, 1.0, 1.0])
    with pytest.raises(BnnHipError, match="strictly increasing"):
        D.PosteriorStats(_cpu_net(), bins=[0.0, 2.0, 1.0])
    with pytest.raises(BnnHipError, match="bin edges"):
        ops.param_hist_args([dict(kind=L.HIST_VALUE, src0=t)], np.arange(L.HIST_MAX_EDGES + 1.0))
    with pytest.raises(BnnHipError, match="bin edges"):
        ops.param_hist_args([dict(kind=L.HIST_VALUE, src0=t)], [0.0])
    with pytest.raises(BnnHipError, match="jobs per call"):
        ops.param_hist_args([dict(kind=L.HIST_VALUE, src0=t)] * (L.HIST_MAX_JOBS + 1), [0.0, 1.0])
    with pytest.raises(BnnHipError, match="jobs per call"):
        ops.param_hist_args([], [0.0, 1.0])
    with pytest.raises(BnnHipError, match="contiguous float32"):
        ops.param_hist_args([dict(kind=L.HIST_VALUE, src0=torch.zeros(4, 4).t())], [0.0, 1.0])
    with pytest.raises(BnnHipError, match="contiguous float32"):
        ops.param_hist_args([dict(kind=L.HIST_VALUE, src0=torch.zeros(4, dtype=torch.float64))], [0.0, 1.0])
    with pytest.raises(BnnHipError, match="contiguous float32"):
        ops.param_hist_args([dict(kind=L.HIST_SNR_DB, src0=t, src1=None)], [0.0, 1.0])
    with pytest.raises(BnnHipError, match="unknown kind"):
        ops.param_hist_args([dict(kind=7, src0=t)], [0.0, 1.0])
    with pytest.raises(BnnHipError, match="no CPU fallback"):
        ops.param_hist_args([dict(kind=L.HIST_VALUE, src0=t)], [0.0, 1.0])
    with pytest.raises(BnnHipError, match="no CPU fallback"):
        D.PosteriorStats(_cpu_net())
    with pytest.raises(BnnHipError, match="no CPU fallback"):
        D.PosteriorStats(torch.nn.Linear(3, 2))
    from bnn_hip import posthoc
    with pytest.raises(BnnHipError, match="no CPU fallback"):
        posthoc.collect_weights(_cpu_net(), bnn=True)
    w = posthoc.collect_weights(torch.nn.Linear(3, 2))                    # no device work: a concatenation
    assert w.shape == (8,)


class _Writer:
    def __init__(self):
        self.hist, self.scalars = [], []

    def add_scalar(self, tag, value, step):
        self.scalars.append((tag, float(value), step))

    def add_histogram_raw(self, tag, min, max, num, sum, sum_squares, bucket_limits, bucket_counts, global_step=None):
        assert len(bucket_limits) == len(bucket_counts)
        self.hist.append((tag, num, global_step))


class _FakeStats:
    built = 0

    def __init__(self, net):
        type(self).built += 1

    def update(self, sample=None):
        return self

    def read(self):
        return {t: dict(min=0.0, max=1.0, num=5, sum=2.0, sum_squares=3.0, bucket_limits=[0.5, 1.0], bucket_counts=[0, 5]) for t in R.TAGS}


def _task(name, tmp_path, monkeypatch, **kw):
    import config
    from bnn_hip import tasks
    monkeypatch.setattr(config, "DEVICE", torch.device("cpu"))         # construction only: nothing is launched
    klass = name.endswith("Classification")
    params = dict(lr=1e-3, hidden_units=8, mode="classification" if klass else "regression", batch_size=4, num_batches=3,
                  train_samples=2, test_samples=3, x_shape=16 if klass else 1, classes=3, y_shape=1, noise_tolerance=0.1,
                  mu_init=[-0.2, 0.2], rho_init=[-5, -4], prior_init=[1.0], mixture_prior=False, local_reparam=False,
                  dropout=True, save_dir=str(tmp_path / "saved"), epochs=1)
    return getattr(tasks, name)(name.lower(), params, **kw)


@pytest.mark.parametrize("name,row", [("BNN_Classification", (10.0, -3.0, -1.0, 6.0)), ("BNN_Regression", (10.0, 4.0, 6.0))])
def test_log_progress_with_histograms_writes_the_reference_tags(name, row, tmp_path, monkeypatch):
    from bnn_hip import diagnostics
    monkeypatch.setattr(diagnostics, "PosteriorStats", _FakeStats)
    _FakeStats.built = 0
    w = _Writer()
    t = _task(name, tmp_path, monkeypatch, writer=w, histograms=True)
    t.loss_info = t._loss_info(torch.tensor(row))
    if name == "BNN_Classification":
        t.acc = 0.5
    t.log_progress(7)
    t.log_progress(8)
    assert _FakeStats.built == 1                                       # planned once
    assert [h[0] for h in w.hist[:12]] == list(R.TAGS) and len(w.hist) == 24 and {h[2] for h in w.hist} == {7, 8}
    first = [s for s in w.scalars if s[2] == 7]
    legacy = [("loss", 10.0, 7)] + ([("accuracy", 0.5, 7)] if name == "BNN_Classification" else [])
    assert first[:len(legacy)] == legacy
    logs = first[len(legacy):]
    if len(row) == 4:                                                  # utils/logger_utils.py:30-35
        assert [s[0] for s in logs] == list(R.SCALARS_4)
        assert [s[1] for s in logs] == [10.0, -1.0 - -3.0, -3.0, -1.0, 6.0]
    else:                                                              # :37-39
        assert [s[0] for s in logs] == list(R.SCALARS_3)
        assert [s[1] for s in logs] == [10.0, 4.0, 6.0]


@pytest.mark.parametrize("name", ["BNN_Classification", "BNN_Regression", "MLP_Classification", "MCDropout_Regression"])
def test_log_progress_without_histograms_is_unchanged(name, tmp_path, monkeypatch):
    from bnn_hip import diagnostics

    def boom(*a, **k):
        raise AssertionError("PosteriorStats must not be built")
    monkeypatch.setattr(diagnostics, "PosteriorStats", boom)
    bayes = name.startswith("BNN")
    for kw in ({}, {"histograms": True}) if not bayes else ({},):      # the non-Bayesian tasks ignore the flag
        w = _Writer()
        t = _task(name, tmp_path, monkeypatch, writer=w, **kw)
        t.loss_info = t._loss_info(torch.tensor((10.0, 4.0, 6.0))) if bayes else torch.tensor(10.0)
        if name.endswith("Classification"):
            t.acc = 0.25
        t.log_progress(3)
        assert w.hist == []
        assert w.scalars == [("loss", 10.0, 3)] + ([("accuracy", 0.25, 3)] if name.endswith("Classification") else [])
    _task(name, tmp_path, monkeypatch).log_progress(0)                 # no writer: a no-op, with or without the flag
    _task(name, tmp_path, monkeypatch, histograms=True).log_progress(0)
