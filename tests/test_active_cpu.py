"""CPU-side checks of device-resident active learning (bnn_acquire_topk / _compose / _random, bnn_hip.active; no GPU): the
entry points exist, the ctypes mirror matches the header, every argument check runs on the host before a launch, the
numpy restatement of the selection order (tests/active_ref.py) agrees with a brute-force Python sort on adversarial
inputs, and the host-side refusals fire."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import active_ref as R
from oracle import bnn_oracle as O
from test_bandit_cpu import _layout

FAKE = 0x10000
NEW = ("bnn_acquire_topk_workspace_bytes", "bnn_acquire_topk", "bnn_acquire_compose", "bnn_acquire_random")


def test_active_exports_and_abi_version():
    import bnn_hip
    from bnn_hip import _lib as L
    lib = L.load()
    assert lib.bnn_version() == 9 == L.ABI_VERSION
    for name in NEW:
        assert name in L.EXPORTS and hasattr(lib, name)
    from bnn_hip import active, ops
    assert bnn_hip.ActivePool is active.ActivePool and bnn_hip.ActiveLearner is active.ActiveLearner
    for name in ("acquire_topk_args", "acquire_topk", "acquire_compose", "acquire_random"):
        assert callable(getattr(ops, name))
    assert active.ACQUISITIONS == ("bald", "entropy", "variance", "random")


def test_active_struct_layout_matches_the_header(tmp_path):
    from bnn_hip import _lib as L
    _layout(tmp_path, L.AcquireTopkArgs, "bnn_acquire_topk_args",
            [("BNN_ACQUIRE_MAX_K", L.ACQUIRE_MAX_K), ("BNN_EPOCH_MAX_ROWS", L.EPOCH_MAX_ROWS), ("BNN_HIP_ABI_VERSION", L.ABI_VERSION)])
    # the winners' 8-byte keys sort in one block's LDS (64 KiB), and the row index fits the key's 16 bits
    assert 8 * L.ACQUIRE_MAX_K <= 64 * 1024 and L.EPOCH_MAX_ROWS <= 1 << 16
    assert L.load().bnn_acquire_topk_workspace_bytes() >= 8 * L.ACQUIRE_MAX_K


def _topk_args(**over):
    from bnn_hip import _lib as L
    a = L.AcquireTopkArgs()
    a.struct_bytes = C.sizeof(L.AcquireTopkArgs)
    a.n_rows, a.k = 100, 7
    for f in ("scores", "candidate", "selected", "labelled", "n_labelled", "n_selected", "workspace"):
        setattr(a, f, FAKE)
    a.workspace_bytes = L.load().bnn_acquire_topk_workspace_bytes()
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_topk_argument_validation_without_a_device():
    """Fake, never dereferenced device addresses: every rejection happens before a launch."""
    from bnn_hip import _lib as L
    fn = L.load().bnn_acquire_topk
    assert fn(None, None) == -1                                                              # BNN_ERR_NULL
    for delta in (8, -8):
        assert fn(C.byref(_topk_args(struct_bytes=C.sizeof(L.AcquireTopkArgs) + delta)), None) == -5   # BNN_ERR_ABI
    for bad in (dict(k=0), dict(k=-1), dict(k=L.ACQUIRE_MAX_K + 1), dict(n_rows=0), dict(n_rows=-5), dict(n_rows=L.EPOCH_MAX_ROWS + 1)):
        assert fn(C.byref(_topk_args(**bad)), None) == -2, bad                               # BNN_ERR_SHAPE
    for f in ("scores", "candidate", "selected", "labelled", "n_labelled"):
        assert fn(C.byref(_topk_args(**{f: None})), None) == -1, f
    assert fn(C.byref(_topk_args(workspace=None)), None) == -4                               # BNN_ERR_WORKSPACE
    assert fn(C.byref(_topk_args(workspace_bytes=L.load().bnn_acquire_topk_workspace_bytes() - 1)), None) == -4
    for f, off in (("scores", 2), ("selected", 2), ("labelled", 1), ("n_labelled", 2), ("n_selected", 2), ("workspace", 4)):
        assert fn(C.byref(_topk_args(**{f: FAKE + off})), None) == -6, f                      # BNN_ERR_ALIGN


def test_compose_and_random_argument_validation_without_a_device():
    from bnn_hip import _lib as L
    lib = L.load()
    for args in ((None, FAKE, FAKE), (FAKE, None, FAKE), (FAKE, FAKE, None)):
        assert lib.bnn_acquire_compose(*args, 10, None) == -1
    for n in (0, -1, L.EPOCH_MAX_ROWS + 1):
        assert lib.bnn_acquire_compose(FAKE, FAKE, FAKE, n, None) == -2
    for args in ((FAKE + 2, FAKE, FAKE), (FAKE, FAKE + 1, FAKE), (FAKE, FAKE, FAKE + 2)):
        assert lib.bnn_acquire_compose(*args, 10, None) == -6
    assert lib.bnn_acquire_random(None, 10, 1, 0, None) == -1
    for n in (0, -1, L.EPOCH_MAX_ROWS + 1):
        assert lib.bnn_acquire_random(FAKE, n, 1, 0, None) == -2
    assert lib.bnn_acquire_random(FAKE + 2, 10, 1, 0, None) == -6


# ------------------------------------------------------------------------------------------------ the order's restatement
def _brute(scores, candidate):
    """The definition, as a comparison sort: score descending, NaN after every number, -0.0 == +0.0, then row ascending."""
    def cmp(i, j):
        a, b = float(scores[i]), float(scores[j])
        na, nb = math.isnan(a), math.isnan(b)
        if na != nb:
            return 1 if na else -1
        if not na and a != b:                     # (-0.0 == 0.0 in Python too)
            return -1 if a > b else 1
        return -1 if i < j else 1
    return sorted([i for i in range(len(scores)) if candidate[i]], key=functools.cmp_to_key(cmp))


def _adversarial():
    rs = np.random.RandomState(3)
    inf, nan = np.inf, np.nan
    yield "ties", (rs.randint(0, 8, 200) / 8).astype(np.float32), np.ones(200, np.uint8)
    yield "specials", np.array([0.0, -0.0, nan, inf, -inf, 1.0, -1.0, nan, 0.0, -0.0, inf, 1e-45, -1e-45, 3.4e38, -3.4e38],
                               np.float32), np.ones(15, np.uint8)
    neg_nan = np.array([0xFFC00001, 0x7F800001, 0x7FFFFFFF, 0xFF800000, 0x80000000, 0x00000000], np.uint32).view(np.float32)
    yield "nan-payloads", neg_nan, np.ones(6, np.uint8)
    s = rs.standard_normal(300).astype(np.float32)
    s[rs.randint(0, 300, 40)] = nan
    s[rs.randint(0, 300, 20)] = 0.0
    s[rs.randint(0, 300, 20)] = -0.0
    yield "mixed", s, (rs.uniform(size=300) < 0.5).astype(np.uint8)
    m = np.zeros(300, np.uint8)
    m[[5, 17, 299]] = 1
    yield "few-left", s, m
    yield "none-left", s, np.zeros(300, np.uint8)
    yield "all-nan", np.full(9, nan, np.float32), np.ones(9, np.uint8)


@pytest.mark.parametrize("name,scores,candidate", list(_adversarial()), ids=[c[0] for c in _adversarial()])
def test_restated_order_equals_a_brute_force_sort(name, scores, candidate):
    want = _brute(scores, candidate)
    assert R.order(scores, candidate).tolist() == want
    n0 = 4
    lab0 = np.full(len(scores) + n0, -7, np.int32)
    for k in (1, 3, max(len(want), 1), len(want) + 2):
        sel, cand, lab, n, m = R.topk(scores, candidate, k, lab0, n0)
        assert m == min(k, len(want)) and n == n0 + m
        assert sel[:m].tolist() == want[:m] and (sel[m:] == -1).all()
        assert cand.sum() == int(np.asarray(candidate).sum()) - m and not cand[sel[:m]].any()
        assert lab[n0:n0 + m].tolist() == want[:m] and (lab[:n0] == -7).all() and (lab[n0 + m:] == -7).all()


def test_rank_key_is_monotone_and_separates_nan():
    v = np.array([np.inf, 3.4e38, 1.0, 1e-45, 0.0, -1e-45, -1.0, -3.4e38, -np.inf], np.float32)
    k = R.rank_key(v).astype(np.int64)
    assert (np.diff(k) > 0).all() and k.max() < 0xFFFFFFFF
    assert R.rank_key(np.array([0.0, -0.0], np.float32)).tolist() == [0x7FFFFFFF] * 2
    assert (R.rank_key(np.array([np.nan, -np.nan], np.float32)) == 0xFFFFFFFF).all()


def test_random_scores_are_the_oracle_philox_words():
    seed, rnd, N = 0x123456789ABCDEF0, 6, 39
    assert R.COUNTER_WORDS == (3, 1)                                                        # off eps (.., 0), the bandit ((0|1), 1), F8 (2, 1)
    s = R.random_scores(seed, rnd, N)
    assert s.dtype == np.float32 and (s >= 0).all() and (s < 1).all() and len(set(s.tolist())) > N // 2
    for i in (0, 1, 2, 3, 4, 38):
        w = O.philox4x32(i >> 2, rnd, 3, 1, seed & 0xFFFFFFFF, seed >> 32)
        assert float(s[i]) == (int(np.asarray(w[i & 3]).reshape(())) >> 8) / 2.0 ** 24
    assert not np.array_equal(s, R.random_scores(seed, rnd + 1, N))
    assert np.array_equal(R.compose([9, 4, 7, 1], [2, 0, 3, 1]), [7, 9, 1, 4])


# ------------------------------------------------------------------------------------------------ host-side refusals
def _pool(N=40, initial=(3, 5, 8), reg=False):
    from bnn_hip import active, epoch
    if reg:
        ds = epoch.DeviceDataset(np.zeros((N, 1), np.float32), np.zeros((N, 1), np.float32), device="cpu")
    else:
        ds = epoch.DeviceDataset(np.zeros((N, 1, 4, 4), np.uint8), np.zeros(N, np.int64), device="cpu")
    return active.ActivePool(ds, list(initial))


def _net(kind, mode):
    import networks
    mp = dict(input_shape=16 if mode == "classification" else 1, classes=3 if mode == "classification" else 1, batch_size=8,
              hidden_units=8, mode=mode)
    if kind == "bnn":
        return networks.BayesianNetwork(dict(mp, mu_init=[-0.2, 0.2], rho_init=[-5, -4], prior_init=[1.0], mixture_prior=False,
                                             local_reparam=False))
    return (networks.MLP if kind == "mlp" else networks.MLP_Dropout)(mp)


def test_pool_bookkeeping_and_the_short_pool_refusal():
    from bnn_hip import _lib as L
    from bnn_hip.ops import BnnHipError
    pool = _pool()
    assert len(pool) == 37 and pool.n_labelled == 3 and pool.labelled.tolist() == [3, 5, 8] and pool.labelled.dtype == torch.int32
    assert pool.candidate.dtype == torch.uint8 and int(pool.candidate.sum()) == 37 and not pool.candidate[[3, 5, 8]].any()
    assert int(pool.n_labelled_word) == 3
    scores = torch.zeros(40)
    with pytest.raises(BnnHipError, match="only 37 candidates"):
        pool.acquire(scores, 38)
    for k in (0, L.ACQUIRE_MAX_K + 1):
        with pytest.raises(BnnHipError, match="BNN_ACQUIRE_MAX_K"):
            pool.acquire(scores, k)
    with pytest.raises(BnnHipError, match="no CPU fallback"):                                # nothing runs off the device
        pool.acquire(scores, 5)
    assert pool.n_labelled == 3 and pool.round == 0                                         # a refused call changes nothing
    with pytest.raises(BnnHipError, match="distinct"):
        _pool(initial=(1, 1))
    with pytest.raises(BnnHipError, match="initial rows"):
        _pool(initial=(40,))
    ld = pool.loader(2, seed=1)
    assert len(ld) == 1
    pool.n_labelled = 7                                                                      # the loader follows the pool's size
    assert len(ld) == 3
    with pytest.raises(BnnHipError, match="batch_size"):
        _pool().loader(4)


def test_acquisitions_are_refused_on_the_host_where_they_do_not_apply():
    from bnn_hip.ops import BnnHipError
    with pytest.raises(BnnHipError, match="classification score"):
        _pool(reg=True).score(_net("bnn", "regression"), 4, "entropy")
    with pytest.raises(BnnHipError, match="classification score"):
        _pool(reg=True).score(_net("dropout", "regression"), 4, "bald")
    with pytest.raises(BnnHipError, match="regression score"):
        _pool().score(_net("bnn", "classification"), 4, "variance")
    with pytest.raises(BnnHipError, match="accepts only 'random'"):
        _pool().score(_net("mlp", "classification"), 4, "bald")
    with pytest.raises(BnnHipError, match="must be one of"):
        _pool().score(_net("bnn", "classification"), 4, "margin")


def test_learner_refuses_uncertainty_scores_on_the_plain_mlp_wrappers(tmp_path, monkeypatch):
    import config
    from bnn_hip import active, tasks
    from bnn_hip.ops import BnnHipError
    monkeypatch.setattr(config, "DEVICE", torch.device("cpu"))         # construction only: nothing is launched
    params = dict(lr=1e-3, hidden_units=8, mode="classification", batch_size=2, num_batches=3, x_shape=16, classes=3,
                  dropout=False, save_dir=str(tmp_path / "saved"), epochs=1)
    t = tasks.MLP_Classification("mlp", params)
    with pytest.raises(BnnHipError, match="accepts only 'random'"):
        active.ActiveLearner(t, _pool(), 4, acquisition="bald", samples=4)
    lrn = active.ActiveLearner(t, _pool(), 4, acquisition="random")
    assert len(lrn.loader) == 1 and lrn.k == 4 and lrn.samples == 0
    with pytest.raises(BnnHipError, match="BNN_ACQUIRE_MAX_K"):
        active.ActiveLearner(t, _pool(), 0, acquisition="random")
