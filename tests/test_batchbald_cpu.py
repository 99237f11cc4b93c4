"""CPU-side checks of BatchBALD (bnn_batchbald_*, bnn_hip.active; include/bnn_hip.h F15; no GPU): the entry points exist
and the ABI version is unchanged, the ctypes mirrors match the header, every `Errors:` line fires on the host before a
launch, the host-side refusals fire, and the numpy restatement (tests/batchbald_ref.py) is itself checked -- the exact form
against a brute-force fp64 enumeration of the definition, step 1 against marg - cond, the sampled estimator against the exact
one within its own standard error."""
import ctypes as C

import numpy as np
import pytest
import torch

import batchbald_ref as R
from test_bandit_cpu import _layout

FAKE = 0x10000
NEW = ("bnn_batchbald_configs", "bnn_batchbald_joint_workspace_bytes", "bnn_batchbald_probs", "bnn_batchbald_joint",
       "bnn_batchbald_begin", "bnn_batchbald_extend")


def test_batchbald_exports_and_abi_version():
    from bnn_hip import _lib as L
    lib = L.load()
    assert lib.bnn_version() == 9 == L.ABI_VERSION
    for name in NEW:
        assert name in L.EXPORTS and hasattr(lib, name)
    from bnn_hip import active, ops
    for name in ("batchbald_probs", "batchbald_joint_args", "batchbald_joint", "batchbald_state_args", "batchbald_begin",
                 "batchbald_extend", "batchbald_configs", "batchbald_joint_workspace"):
        assert callable(getattr(ops, name))
    assert active.ACQUISITIONS == ("bald", "entropy", "variance", "random") and active.BATCH_ACQUISITIONS == ("batchbald",)
    assert callable(active.ActivePool.joint_probs) and callable(active.ActivePool.acquire_batchbald)


def test_batchbald_struct_layouts_match_the_header(tmp_path):
    from bnn_hip import _lib as L
    _layout(tmp_path, L.BatchBaldProbsArgs, "bnn_batchbald_probs_args",
            [("BNN_BATCHBALD_MAX_CLASSES", L.BATCHBALD_MAX_CLASSES), ("BNN_BATCHBALD_MAX_SAMPLES", L.BATCHBALD_MAX_SAMPLES),
             ("BNN_BATCHBALD_MAX_K", L.BATCHBALD_MAX_K), ("BNN_BATCHBALD_MAX_CONFIGS", L.BATCHBALD_MAX_CONFIGS),
             ("BNN_HIP_ABI_VERSION", L.ABI_VERSION)])
    _layout(tmp_path, L.BatchBaldJointArgs, "bnn_batchbald_joint_args")
    _layout(tmp_path, L.BatchBaldStateArgs, "bnn_batchbald_state_args")
    assert L.BATCHBALD_MAX_K < 1 << 8                                       # j takes 8 bits of the label stream's counter
    assert 64 * (L.BATCHBALD_MAX_SAMPLES + 4) * 4 <= 64 * 1024               # the joint kernel's Phat tile fits a block's LDS


def test_configs_and_workspace_are_host_functions():
    from bnn_hip import _lib as L
    from bnn_hip import ops
    lib = L.load()
    for Cc, mc in ((3, 27), (3, 26), (2, 65536), (10, 8192), (32, 1), (5, 4)):
        for n in (0, 1, 2, 3, 4, 6, 16, 17, 64):
            want = Cc ** n if Cc ** n <= mc else mc
            assert lib.bnn_batchbald_configs(Cc, n, mc) == want == ops.batchbald_configs(Cc, n, mc) == R.configs(Cc, n, mc)
    for bad in ((1, 1, 8), (33, 1, 8), (3, -1, 8), (3, 65, 8), (3, 1, 0), (3, 1, 65537)):
        assert lib.bnn_batchbald_configs(*bad) == 0
    ws = lib.bnn_batchbald_joint_workspace_bytes
    assert ws(37, 3, 1) == 8 * 37 and ws(60000, 10, 8192) == 8 * 60000                 # a pool that fills the chip is not split
    assert ws(37, 3, 8192) > 8 * 37 and ws(37, 3, 8192) % (8 * 37) == 0                # a small one is, over M
    for bad in ((0, 3, 1), (65537, 3, 1), (5, 1, 1), (5, 33, 1), (5, 3, 0), (5, 3, 65537)):
        assert ws(*bad) == 0


def _args(cls, fields, **over):
    a = cls()
    a.struct_bytes = C.sizeof(cls)
    for f in fields:
        setattr(a, f, FAKE)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _probs_args(**over):
    from bnn_hip import _lib as L
    return _args(L.BatchBaldProbsArgs, ("logits", "probs", "cond", "marg"),
                 **dict(dict(n_samples=4, n_rows=100, n_classes=3, row0=10, chunk_rows=20), **over))


def _joint_args(**over):
    from bnn_hip import _lib as L
    d = dict(n_samples=4, n_rows=100, n_classes=3, n_configs=27, workspace_bytes=1 << 20)
    return _args(L.BatchBaldJointArgs, ("probs", "phat", "weight", "offset", "cond", "base", "scores", "scores64", "joint64", "workspace"),
                 **dict(d, **over))


STATE_PTRS = ("probs", "cond", "labelled", "n_labelled", "scores64", "phat_in", "expo_in", "phat_out", "expo_out", "weight", "offset",
              "base", "batch_scores")


def _state_args(**over):
    from bnn_hip import _lib as L
    d = dict(n_samples=4, n_rows=100, n_classes=3, max_configs=27, n_chosen=2, round=1, seed=7)
    return _args(L.BatchBaldStateArgs, STATE_PTRS, **dict(d, **over))


DIMS = (dict(n_classes=1), dict(n_classes=33), dict(n_samples=0), dict(n_samples=129), dict(n_rows=0), dict(n_rows=65537))


def test_probs_argument_validation_without_a_device():
    """Fake, never dereferenced device addresses: every rejection happens before a launch."""
    from bnn_hip import _lib as L
    fn = L.load().bnn_batchbald_probs
    assert fn(None, None) == -1
    for delta in (8, -8):
        assert fn(C.byref(_probs_args(struct_bytes=C.sizeof(L.BatchBaldProbsArgs) + delta)), None) == -5
    for bad in DIMS + (dict(chunk_rows=0), dict(row0=-1), dict(row0=81), dict(row0=100, chunk_rows=1)):
        assert fn(C.byref(_probs_args(**bad)), None) == -2, bad
    for f in ("logits", "probs", "cond", "marg"):
        assert fn(C.byref(_probs_args(**{f: None})), None) == -1, f
    for f, off in (("logits", 2), ("probs", 2), ("cond", 4), ("marg", 4)):
        assert fn(C.byref(_probs_args(**{f: FAKE + off})), None) == -6, f


def test_joint_argument_validation_without_a_device():
    from bnn_hip import _lib as L
    lib = L.load()
    fn = lib.bnn_batchbald_joint
    assert fn(None, None) == -1
    for delta in (8, -8):
        assert fn(C.byref(_joint_args(struct_bytes=C.sizeof(L.BatchBaldJointArgs) + delta)), None) == -5
    for bad in DIMS + (dict(n_configs=0), dict(n_configs=65537)):
        assert fn(C.byref(_joint_args(**bad)), None) == -2, bad
    for f in ("probs", "phat", "weight", "offset", "cond", "base", "scores"):
        assert fn(C.byref(_joint_args(**{f: None})), None) == -1, f
    assert fn(C.byref(_joint_args(workspace=None)), None) == -4
    assert fn(C.byref(_joint_args(workspace_bytes=lib.bnn_batchbald_joint_workspace_bytes(100, 3, 27) - 1)), None) == -4
    for f, off in (("probs", 2), ("phat", 2), ("scores", 2), ("weight", 4), ("offset", 4), ("cond", 4), ("base", 4), ("scores64", 4),
                   ("joint64", 4), ("workspace", 4)):
        assert fn(C.byref(_joint_args(**{f: FAKE + off})), None) == -6, f


def test_begin_and_extend_argument_validation_without_a_device():
    from bnn_hip import _lib as L
    lib = L.load()
    size = C.sizeof(L.BatchBaldStateArgs)
    for fn in (lib.bnn_batchbald_begin, lib.bnn_batchbald_extend):
        assert fn(None, None) == -1
        for delta in (8, -8):
            assert fn(C.byref(_state_args(struct_bytes=size + delta)), None) == -5
    begin, extend = lib.bnn_batchbald_begin, lib.bnn_batchbald_extend
    for bad in (dict(n_samples=0), dict(n_samples=129)):
        assert begin(C.byref(_state_args(**bad)), None) == -2, bad
    for f in ("phat_out", "expo_out", "weight", "offset", "base"):
        assert begin(C.byref(_state_args(**{f: None})), None) == -1, f
    for f, off in (("phat_out", 2), ("expo_out", 2), ("weight", 4), ("offset", 4), ("base", 4)):
        assert begin(C.byref(_state_args(**{f: FAKE + off})), None) == -6, f
    for bad in DIMS + (dict(max_configs=0), dict(max_configs=65537), dict(n_chosen=0), dict(n_chosen=65)):
        assert extend(C.byref(_state_args(**bad)), None) == -2, bad
    for f in STATE_PTRS:
        if f not in ("scores64", "batch_scores"):
            assert extend(C.byref(_state_args(**{f: None})), None) == -1, f
    assert extend(C.byref(_state_args(scores64=None)), None) == -1                      # batch_scores needs the step's scores
    for f in STATE_PTRS:
        off = 4 if f in ("cond", "scores64", "weight", "offset", "base", "batch_scores") else 2
        assert extend(C.byref(_state_args(**{f: FAKE + off})), None) == -6, f


# ------------------------------------------------------------------------------------------------ host-side refusals
def _pool(N=40, initial=(3, 5, 8)):
    from bnn_hip import active, epoch
    ds = epoch.DeviceDataset(np.zeros((N, 1, 4, 4), np.uint8), np.zeros(N, np.int64), device="cpu")
    return active.ActivePool(ds, list(initial))


def _net(kind, mode="classification", lr=False):
    import networks
    mp = dict(input_shape=16 if mode == "classification" else 1, classes=3 if mode == "classification" else 1, batch_size=8,
              hidden_units=8, mode=mode)
    if kind == "bnn":
        return networks.BayesianNetwork(dict(mp, mu_init=[-0.2, 0.2], rho_init=[-5, -4], prior_init=[1.0], mixture_prior=False,
                                             local_reparam=lr))
    return (networks.MLP if kind == "mlp" else networks.MLP_Dropout)(mp)


def test_joint_probs_is_refused_on_the_host_where_weight_draws_are_not_shared():
    import bnn_hip
    from bnn_hip.ops import BnnHipError
    from bnn_hip.runtime import state
    with pytest.raises(BnnHipError, match="per row"):
        _pool().joint_probs(_net("bnn", lr=True), 4)
    with pytest.raises(BnnHipError, match="per row"):
        _pool().joint_probs(_net("dropout"), 4)
    with pytest.raises(BnnHipError, match="accepts only 'random'"):
        _pool().joint_probs(_net("mlp"), 4)
    with pytest.raises(BnnHipError, match="classification score"):
        _pool().joint_probs(_net("bnn", "regression"), 4)
    bnn_hip.shard_samples(True)
    try:
        with pytest.raises(BnnHipError, match="sharding"):
            _pool().joint_probs(_net("bnn"), 4)
    finally:
        bnn_hip.shard_samples(False)
    bnn_hip.set_host_eps(True)                                                              # drawn afresh by every forward_mc call
    try:
        with pytest.raises(BnnHipError, match="drawn afresh"):
            _pool().joint_probs(_net("bnn"), 4)
    finally:
        bnn_hip.set_host_eps(False)
    stubbed = _net("bnn")
    stubbed.l2.weight.normal = object()                                                     # the identical-epsilon seam of the parity tests
    with pytest.raises(BnnHipError, match="drawn afresh"):
        _pool().joint_probs(stubbed, 4)
    c = state.counter
    for S in (0, 129):
        with pytest.raises(BnnHipError, match="BNN_BATCHBALD_MAX_SAMPLES"):
            _pool().joint_probs(_net("bnn"), S)
    with pytest.raises(BnnHipError, match="no CPU fallback"):                                # nothing runs off the device
        _pool().joint_probs(_net("bnn"), 4)
    assert state.counter == c                                                               # a refused call takes no samples


def test_acquire_batchbald_refusals_and_names():
    from bnn_hip import active
    from bnn_hip.ops import BnnHipError
    pool = _pool()
    joint = active.JointProbs(torch.zeros((4, 40, 3)), torch.zeros(40, dtype=torch.float64), torch.zeros(40, dtype=torch.float64), 0)
    for k in (0, 65):
        with pytest.raises(BnnHipError, match="BNN_BATCHBALD_MAX_K"):
            pool.acquire_batchbald(joint, k)
    for mc in (0, 65537):
        with pytest.raises(BnnHipError, match="BNN_BATCHBALD_MAX_CONFIGS"):
            pool.acquire_batchbald(joint, 3, max_configs=mc)
    with pytest.raises(BnnHipError, match="only 37 candidates"):
        pool.acquire_batchbald(joint, 38)
    with pytest.raises(BnnHipError, match="one row of probabilities"):
        pool.acquire_batchbald(active.JointProbs(torch.zeros((4, 39, 3)), None, None, 0), 3)
    with pytest.raises(BnnHipError, match="no CPU fallback"):
        pool.acquire_batchbald(joint, 3)
    assert pool.n_labelled == 3 and pool.round == 0                                         # a refused call changes nothing
    with pytest.raises(BnnHipError, match="scores a batch jointly"):
        pool.score(_net("bnn"), 4, "batchbald")
    with pytest.raises(BnnHipError, match="must be one of"):
        active.check_acquisition(_net("bnn"), "batchbalt")
    active.check_acquisition(_net("bnn"), "batchbald")
    with pytest.raises(BnnHipError, match="per row"):
        active.check_acquisition(_net("bnn", lr=True), "batchbald")


def test_learner_checks_the_batchbald_limits_at_construction(tmp_path, monkeypatch):
    import config
    from bnn_hip import active, tasks
    from bnn_hip.ops import BnnHipError
    monkeypatch.setattr(config, "DEVICE", torch.device("cpu"))         # construction only: nothing is launched
    params = dict(lr=1e-3, hidden_units=8, mode="classification", batch_size=2, num_batches=3, train_samples=2, test_samples=4,
                  x_shape=16, classes=3, mu_init=[-0.2, 0.2], rho_init=[-5, -4], prior_init=[1.0], mixture_prior=False,
                  local_reparam=False, dropout=False, save_dir=str(tmp_path / "saved"), epochs=1)
    t = tasks.BNN_Classification("bnn", params)
    lrn = active.ActiveLearner(t, _pool(), 3, acquisition="batchbald", max_configs=64)
    assert lrn.samples == 4 and lrn.max_configs == 64 and lrn.k == 3
    with pytest.raises(BnnHipError, match="BNN_BATCHBALD_MAX_K"):
        active.ActiveLearner(t, _pool(N=200), 65, acquisition="batchbald")
    with pytest.raises(BnnHipError, match="BNN_BATCHBALD_MAX_SAMPLES"):
        active.ActiveLearner(t, _pool(), 3, acquisition="batchbald", samples=129)
    active.ActiveLearner(t, _pool(), 3, acquisition="bald", samples=129)                    # the per-row scores have no such limit


# ------------------------------------------------------------------------------------------------ the restatement itself
def _problem(S, N, C, seed, sharp=3.0):
    rs = np.random.RandomState(seed)
    z = sharp * rs.standard_normal((S, N, C))
    p = np.exp(z - z.max(axis=2, keepdims=True))
    P = (p / p.sum(axis=2, keepdims=True)).astype(np.float32)
    cond, marg = R.entropies(P)
    return P, cond, marg


def test_ln2_and_rescaling_are_exact():
    import math
    assert R.LN2 == math.log(2.0) == float(np.log(2.0))
    rows = np.array([[1e-12, 3e-20, 0.0], [0.0, 0.0, 0.0], [1.0, 0.5, 1e-45], [0.75, 0.1, 0.2]], np.float32)
    out, e = R.rescale(rows)
    assert e.tolist() == [-39, 0, 1, 0] and out.dtype == np.float32
    assert 0.5 <= out[0].max() < 1 and not out[1].any() and 0.5 <= out[2].max() < 1
    assert np.array_equal(np.ldexp(out[[0, 1, 3]].astype(np.float64), e[[0, 1, 3], None]), rows[[0, 1, 3]].astype(np.float64))


def test_step_one_is_plain_bald():
    P, cond, marg = _problem(4, 7, 3, 1)
    st = R.begin(4)
    np.testing.assert_allclose(R.joint(st, P), marg, rtol=0, atol=1e-15)
    np.testing.assert_allclose(R.scores(st, P, cond), marg - cond, rtol=0, atol=1e-15)


def test_exact_form_equals_a_brute_force_enumeration_of_the_definition():
    """C = 3, S = 4, N = 7, up to 4 chosen rows: H from (Phat, E, w, o) against - sum p log p over every label tuple, in
    fp64.  Phat is fp32: each factor rounds once (2^-24 relative), so 5 factors stay within 1e-6 of the fp64 product."""
    S, N, C = 4, 7, 3
    P, cond, _ = _problem(S, N, C, 2)
    st, chosen = R.begin(S), []
    for i in (5, 0, 3, 6):
        chosen.append(i)
        st = R.extend(st, P, cond, chosen, max_configs=3 ** 4)
        assert st.M == C ** len(chosen) and np.array_equal(st.w, np.ldexp(1.0, st.E)) and st.base == pytest.approx(cond[chosen].sum())
        assert ((st.phat.max(axis=1) >= 0.5) & (st.phat.max(axis=1) < 1)).all()
        H = R.joint(st, P)
        for cand in range(N):
            if cand not in chosen:
                assert H[cand] == pytest.approx(R.brute_joint_entropy(P, chosen, cand), rel=1e-6), (chosen, cand)


def test_tiny_probabilities_do_not_underflow():
    """Entries of 1e-12: five factors are 1e-60, far below fp32; the rescaled rows keep them and E carries the scale."""
    S, N, C = 4, 6, 3
    P = np.full((S, N, C), 1e-12, np.float32)
    P[:, :, 2] = 1.0
    P[0, :, 0] = 0.0                                                  # exact zeros too
    cond, _ = R.entropies(P)
    st, chosen = R.begin(S), []
    for i in range(5):
        chosen.append(i)
        st = R.extend(st, P, cond, chosen, max_configs=3 ** 5)
    assert st.E.min() < -150 and st.phat.max(axis=1).min() >= 0.5      # no row lost (only s = 0 entries are zero)
    H = R.joint(st, P)
    assert np.isfinite(H).all() and H[5] == pytest.approx(R.brute_joint_entropy(P, chosen, 5), rel=1e-6, abs=1e-18)


def test_labels_are_a_pure_function_of_seed_round_row_and_step():
    S, N, C, M = 4, 7, 3, 64
    P, _, _ = _problem(S, N, C, 3)
    sm = np.arange(M) % S
    a = R.labels(11, 2, 1, P[sm, 4, :])
    assert np.array_equal(a, R.labels(11, 2, 1, P[sm, 4, :])) and a.min() >= 0 and a.max() <= C - 1
    assert not np.array_equal(a, R.labels(11, 3, 1, P[sm, 4, :])) and not np.array_equal(a, R.labels(11, 2, 2, P[sm, 4, :]))
    assert not np.array_equal(a, R.labels(12, 2, 1, P[sm, 4, :]))
    one_hot = np.zeros((M, C), np.float32)
    one_hot[:, 1] = 1.0
    assert (R.labels(11, 2, 1, one_hot) == 1).all()                                       # a zero-probability class is never drawn
    # the first sampled step rebuilds from ones what one factor per step gives afterwards: [2] then 5 == [2, 5] at once
    cond = np.zeros(N)
    one = R.extend(R.begin(S), P, cond, [2], max_configs=2, seed=11, rnd=2)               # 3 > 2: sampled from the first step on
    two = R.extend(one, P, cond, [2, 5], max_configs=2, seed=11, rnd=2)                   # continuation: one more factor
    ex = R.extend(R.begin(S), P, cond, [2], max_configs=8, seed=11, rnd=2)                # 3 <= 8: enumerated
    both = R.extend(ex, P, cond, [2, 5], max_configs=8, seed=11, rnd=2)                   # 9 > 8: rebuilt from ones, both factors
    assert one.M == two.M == 2 and ex.M == 3 and both.M == 8
    for f in ("phat", "E", "w", "o"):
        assert np.array_equal(getattr(two, f), getattr(both, f)[:2]) == (f in ("phat", "E", "o")), f   # w holds 1 / M


def test_sampled_estimator_agrees_with_the_exact_one_within_five_standard_errors():
    """S = 8, C = 3, eight chosen rows, M = 4096 sampled configurations against the 6561 enumerated ones, seed 2026, round 0.
    H_est[i] is the mean over m of M w[m] terms[m, i]; its standard error is std / sqrt(M) of those per-row values (the
    rows are stratified over the draws s, which can only lower the variance).  Deterministic.  Observed: the largest
    |H_est - H_exact| / SE over the four candidates is 0.28, the largest relative difference 8.1e-4."""
    S, N, C, M, seed = 8, 12, 3, 4096, 2026
    P, cond, _ = _problem(S, N, C, 5, sharp=1.5)
    chosen = [1, 4, 7, 9, 10, 0, 3, 6]
    ex = sm = R.begin(S)
    for n in range(1, 9):
        ex = R.extend(ex, P, cond, chosen[:n], max_configs=3 ** 8)
        sm = R.extend(sm, P, cond, chosen[:n], max_configs=M, seed=seed, rnd=0)          # 3^8 > 4096: the last step samples
    assert ex.M == 6561 and sm.M == M and (sm.w > 0).all()
    per_row = (M * sm.w)[:, None] * R.terms(sm, P)                       # [M, N]
    est, se = per_row.mean(axis=0), per_row.std(axis=0, ddof=1) / np.sqrt(M)
    np.testing.assert_allclose(est, R.joint(sm, P), rtol=1e-12)
    want = R.joint(ex, P)
    cand = [i for i in range(N) if i not in chosen]
    ratio = np.abs(est - want)[cand] / se[cand]
    print("sampled vs exact: |diff| / SE", ratio.round(2), "relative", (np.abs(est - want)[cand] / want[cand]).max())
    assert (ratio <= 5.0).all(), ratio
