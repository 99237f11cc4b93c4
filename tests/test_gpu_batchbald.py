"""BatchBALD on an MI355X (bnn_batchbald_*, ActivePool.joint_probs / acquire_batchbald; include/bnn_hip.h F15) against the
numpy restatement tests/batchbald_ref.py: the fused joint-entropy kernel within a derived fp32 bound, the state update bit
for bit, the whole greedy loop teacher-forced on the device's own winners, the shared weight draws of joint_probs, and
rounds of ActiveLearner(acquisition="batchbald") without a host synchronisation."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import batchbald_ref as R
import bnn_hip
from bnn_hip import active, epoch, ops
from bnn_hip.runtime import state

SEED = 0x5EED0123456789AB


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore():
    yield
    bnn_hip.set_math("bf16")
    bnn_hip.manual_seed(2026)


def _probs(S, N, C, seed, tiny=False):
    """fp32 P [S, N, C]: softmax rows, with exact zeros (one class of row 0 under every draw, single entries elsewhere) and
    entries of 1e-12; `tiny`: EVERY entry near 1e-12, so an unscaled product of four factors is 1e-48 -- zero in fp32;
    S = 1: dyadic rows k / 256, 1 - k / 256 that sum to exactly 1 and whose products are exact."""
    rs = np.random.RandomState(seed)
    if S == 1:
        k = rs.randint(0, 257, (1, N, 1)).astype(np.float32)
        k[0, 0, 0], k[0, 1, 0] = 0.0, 256.0                  # exact zeros of either class
        P = np.concatenate([k, 256 - k] + [np.zeros_like(k)] * (C - 2), axis=2) / np.float32(256)
        return P.astype(np.float32)
    z = 2.0 * rs.standard_normal((S, N, C))
    p = np.exp(z - z.max(axis=2, keepdims=True))
    P = (p / p.sum(axis=2, keepdims=True)).astype(np.float32)
    if tiny:
        P = (1e-12 * (1.0 + 0.5 * rs.uniform(size=(S, N, C)))).astype(np.float32)
    P[:, 0, 0] = 0.0                                          # label 0 of row 0 is impossible: all-zero Phat rows once row 0 is chosen
    P[0, 1 % N, 1] = 0.0
    P[S - 1, 2 % N, C - 1] = 1e-12
    P[0, 3 % N, 0] = 1e-12
    return P


def _state(P, cond, chosen, max_configs, seed=SEED, rnd=3):
    st = R.begin(P.shape[0])
    for n in range(1, len(chosen) + 1):
        st = R.extend(st, P, cond, chosen[:n], max_configs, seed, rnd)
    return st


def _dev_state(st, dev):
    return (torch.from_numpy(st.phat).to(dev), torch.from_numpy(st.w).to(dev), torch.from_numpy(st.o).to(dev),
            torch.tensor([float(st.base)], dtype=torch.float64, device=dev))


# ---------------------------------------------------------------------------------------------------- 1. the joint kernel
JOINT_CASES = {   # name -> (C, S, N, chosen rows, max_configs) -> M
    "M1": (3, 4, 37, [], 27),                       # the empty batch: plain BALD
    "M27": (3, 4, 37, [0, 5, 36], 27),              # every configuration, nine of them all-zero rows (row 0, label 0)
    "M29": (3, 4, 37, [0, 5, 36, 17], 29),          # 81 > 29: sampled, M no multiple of anything
    "S1": (2, 1, 20, [0, 3, 7], 8),                 # one draw: no mutual information, every score 0
    "M1000-exact": (10, 16, 130, [0, 64, 129], 1000),
    "M1000-sampled": (10, 16, 130, [0, 64, 129, 77], 1000),
    "limits": (32, 128, 5, [1], 3),                 # S and C at their limits; 32 > 3: sampled
    # more than one 64-row tile of Phat per block (every pool that fills the chip): the loop's barrier, the restaged tile and
    # the sum carried across tiles -- 2 050 row blocks, so M is not split: one block walks all three tiles ...
    "tiles3": (32, 4, 4100, [0, 5], 130),
    # ... and 1 050 row blocks: two splits of three and two tiles, the last one short (300 = 4 x 64 + 44); S = 20: two MFMA groups
    "tiles3+2": (32, 20, 2100, [0, 5], 300),
}
TILES = {"tiles3": 1, "tiles3+2": 2}               # name -> splits (bnn_batchbald_joint_workspace_bytes / (8 N))


@pytest.mark.parametrize("name", sorted(JOINT_CASES))
def test_joint_kernel_against_the_restatement(dev, name):
    """|H_dev - H_ref| <= (S + 4) 2^-23 (1 + |H_ref|), H_ref the fp64 restatement from the same fp32 P and Phat.
    Derivation: every term of the sum over s is non-negative, so an fp32 chain of S terms has relative error at most
    S 2^-24 on pt; d(p log p) = (1 + log p) dp and sum p |1 + log p| <= 1 + H turn that into S 2^-24 (1 + H) on H; an fp32
    log adds H 2^-24; the factor 2 covers qt in the sampled weights.  Nothing here was tuned on the device's figures (measured afterwards on
    an MI355X: 3.9e-8 .. 1.3e-7, 0.1 % .. 3.9 % of the bound over the first seven cases).
    Also: scores64 = joint64 - cond - base and scores = fl32(scores64) exactly, no NaN, two launches give the same bits."""
    C, S, N, chosen, mc = JOINT_CASES[name]
    P = _probs(S, N, C, 7)
    cond, _ = R.entropies(P)
    st = _state(P, cond, chosen, mc)
    assert st.M == R.configs(C, len(chosen), mc)
    if name in TILES:                                          # the plan this case is here for: fewer splits than tiles
        from bnn_hip import _lib as L
        assert L.load().bnn_batchbald_joint_workspace_bytes(N, C, st.M) == 8 * N * TILES[name] and -(-st.M // 64) > TILES[name]
    if name == "M27":
        assert (st.phat.max(axis=1) == 0).sum() == 9
    Pd, condd = torch.from_numpy(P).to(dev), torch.from_numpy(cond).to(dev)
    phat, w, o, base = _dev_state(st, dev)
    runs = []
    for _ in range(2):
        sc = torch.full((N,), float("nan"), dtype=torch.float32, device=dev)
        sc64, j64 = (torch.full((N,), float("nan"), dtype=torch.float64, device=dev) for _ in range(2))
        ws = ops.batchbald_joint_workspace(N, C, st.M, dev)
        ws.fill_(float("nan"))                                 # any contents
        ops.batchbald_joint(ops.batchbald_joint_args(probs=Pd, phat=phat, weight=w, offset=o, cond=condd, base=base, scores=sc,
                                                     scores64=sc64, joint64=j64, n_configs=st.M, workspace=ws))
        runs.append([t.cpu().numpy() for t in (sc, sc64, j64)])
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    sc, sc64, j64 = runs[0]
    assert np.isfinite(sc).all() and np.isfinite(sc64).all() and np.isfinite(j64).all()
    H = R.joint(st, P)
    err, bnd = np.abs(j64 - H), R.bound(S, H)
    print(f"{name}: M = {st.M}, largest |H_dev - H_ref| {err.max():.3e}, {(err / bnd).max():.3f} of the bound; H up to {H.max():.3f}")
    assert (err <= bnd).all(), (err / bnd).max()
    assert np.array_equal(sc64, j64 - cond - st.base) and np.array_equal(sc, sc64.astype(np.float32))
    if name == "S1":
        assert (np.abs(sc64) <= bnd).all()
    if name == "M1":
        _, marg = R.entropies(P)
        assert (np.abs(sc64 - (marg - cond)) <= bnd).all()


# ---------------------------------------------------------------------------------------------------- 2. the state update
@pytest.mark.parametrize("tiny", [False, True], ids=["softmax", "1e-12"])
def test_extend_equals_the_restatement_bit_for_bit(dev, tiny):
    """C = 3, S = 4, max_configs = 27, six chosen rows: n = 1, 2, 3 enumerate (3, 9, 27 rows), n = 4 abandons enumeration
    and rebuilds 27 sampled rows from ones, n = 5 and 6 add one factor each.  Phat, E, w, o and base are compared as bits,
    batch_scores[n - 1] is the winner's entry of scores64; a seventh extend with `last` set books base and batch_scores only.  `1e-12`: the unscaled product of four factors would be zero."""
    C, S, N, mc, rnd = 3, 4, 37, 27, 5
    P = _probs(S, N, C, 11, tiny=tiny)
    cond, _ = R.entropies(P)
    chosen = [0, 9, 36, 4, 20, 2]
    final = 15                                                 # a seventh row, folded in with `last` set
    n0 = 3
    lab = np.full(N, -9, np.int32)
    lab[:n0] = [30, 31, 32]
    lab[n0:n0 + len(chosen) + 1] = chosen + [final]
    Pd, condd, labd = torch.from_numpy(P).to(dev), torch.from_numpy(cond).to(dev), torch.from_numpy(lab).to(dev)
    sc64 = torch.from_numpy(np.random.RandomState(1).standard_normal(N)).to(dev)
    phat = [torch.full((mc, S), float("nan"), dtype=torch.float32, device=dev) for _ in range(2)]
    expo = [torch.full((mc,), -77, dtype=torch.int32, device=dev) for _ in range(2)]
    w, o = (torch.full((mc,), float("nan"), dtype=torch.float64, device=dev) for _ in range(2))
    base = torch.full((1,), float("nan"), dtype=torch.float64, device=dev)
    bs = torch.full((len(chosen) + 1,), float("nan"), dtype=torch.float64, device=dev)
    word = torch.tensor([n0], dtype=torch.int32, device=dev)

    def args(n):
        return ops.batchbald_state_args(probs=Pd, cond=condd, labelled=labd, n_labelled=word, phat_in=phat[(n + 1) & 1],
                                        expo_in=expo[(n + 1) & 1], phat_out=phat[n & 1], expo_out=expo[n & 1], weight=w, offset=o,
                                        base=base, max_configs=mc, n_chosen=n, round=rnd, seed=SEED, scores64=sc64,
                                        batch_scores=bs if n else None, last=n > len(chosen))

    def same(st, n):
        M = st.M
        for got, want, what in ((phat[n & 1][:M], st.phat, "Phat"), (expo[n & 1][:M], st.E, "E"), (w[:M], st.w, "w"), (o[:M], st.o, "o"),
                                (base, np.array([st.base]), "base")):
            g = got.cpu().numpy()
            assert g.dtype == want.dtype and np.array_equal(g.view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), (n, what)

    ops.batchbald_begin(args(0))
    st = R.begin(S)
    same(st, 0)
    for n in range(1, len(chosen) + 1):
        word.fill_(n0 + n)
        ops.batchbald_extend(args(n))
        st = R.extend(st, P, cond, chosen[:n], mc, SEED, rnd)
        assert st.M == (3 ** n if n <= 3 else mc)
        same(st, n)
        assert np.isfinite(st.w).all() and np.isfinite(st.o).all()
    # the last row of a batch: base and batch_scores move on, the state of n = 6 stays as it is (in its own half)
    n = len(chosen) + 1
    word.fill_(n0 + n)
    ops.batchbald_extend(args(n))
    same(R.State(st.phat, st.E, st.w, st.o, np.float64(st.base + cond[final])), n - 1)
    assert np.array_equal(bs.cpu().numpy(), sc64.cpu().numpy()[chosen + [final]])
    if tiny:
        assert st.E.max() < -150 and (st.phat.max(axis=1) >= 0.5).all()          # the scale lives in E, no row vanished


# ---------------------------------------------------------------------------------------------------- 3. the greedy loop
@pytest.mark.parametrize("C,S,N,mc,k", [(3, 4, 37, 27, 6), (10, 16, 130, 1000, 5)], ids=["3x4-27", "10x16-1000"])
def test_greedy_loop_teacher_forced_on_the_device_winners(dev, C, S, N, mc, k):
    """acquire_batchbald end to end.  The restatement follows the device's own winners; at every step the winner must be a
    candidate whose reference score is within twice the joint kernel's bound (one bound each for the two rows compared) of
    the reference maximum over the remaining candidates, and batch_scores[n - 1] is that row's reference score within the
    bound.  The mask, the labelled list and the count word are the top-k entry's, checked against the winners."""
    P = _probs(S, N, C, 13)
    cond, marg = R.entropies(P)
    initial = [3, 11, 2]
    X = np.zeros((N, 1, 1, 4), np.float32)
    pool = active.ActivePool(epoch.DeviceDataset(X, np.zeros(N, np.int64), device=dev), initial)
    pool.round = 2
    joint = active.JointProbs(torch.from_numpy(P).to(dev), torch.from_numpy(cond).to(dev), torch.from_numpy(marg).to(dev), 0)
    res = pool.acquire_batchbald(joint, k, max_configs=mc, seed=SEED)
    assert pool.n_labelled == len(initial) + k == int(pool.n_labelled_word.item()) and pool.round == 3
    sel, bs = res.selected.cpu().numpy(), res.batch_scores.cpu().numpy()
    assert sel.dtype == np.int32 and bs.dtype == np.float64 and len(set(sel.tolist())) == k
    cand = np.ones(N, bool)
    cand[initial] = False
    st, chosen = R.begin(S), []
    for n in range(1, k + 1):
        H = R.joint(st, P)
        sc = H - cond - st.base
        w = int(sel[n - 1])
        bnd = R.bound(S, H)
        assert 0 <= w < N and cand[w], (n, w)
        best = sc[cand].max()
        print(f"step {n}: M = {st.M}, winner {w}, reference score {sc[w]:.9f}, best {best:.9f}, device {bs[n - 1]:.9f}")
        assert sc[w] >= best - 2 * bnd[cand].max(), (n, w, sc[w], best)
        assert abs(bs[n - 1] - sc[w]) <= bnd[w], (n, bs[n - 1], sc[w])
        cand[w] = False
        chosen.append(w)
        st = R.extend(st, P, cond, chosen, mc, SEED, 2)
    assert np.array_equal(pool.candidate.cpu().numpy().astype(bool), cand)
    assert pool.labelled.cpu().numpy().tolist() == initial + chosen


# ---------------------------------------------------------------------------------------------------- 4. joint_probs
def _bnn(dev, dims, B, seed):
    import networks
    torch.manual_seed(seed)
    mp = dict(input_shape=dims[0], classes=dims[2], batch_size=B, hidden_units=dims[1], mode="classification", mu_init=[-0.2, 0.2],
              rho_init=[-2, -1], prior_init=[1.0], mixture_prior=False, local_reparam=False)
    return networks.BayesianNetwork(mp).to(dev).train()


def test_joint_probs_shares_weight_draws_across_calls(dev):
    """f32 math, a 16-8-8-3 network, 96 rows evaluated 32 per call: probs against softmax(forward_mc(all 96 rows)) at the
    same first sample index, atol 1e-3 (launch plans may differ with the batch; unshared draws differ at the 0.1 level).
    The counter advances by exactly S.  cond and marg are the fp64 entropies of the returned fp32 probs; the step-1 scores
    equal marg - cond and F3's mutual_information computed from the same probabilities, within the joint kernel's bound.
    Measured on an MI355X: shared draws differ by 6.0e-8, the next S draws by 0.36; step 1 against F3 by 1.8e-7 (bound 3.0e-6)."""
    S, N, dims = 8, 96, (16, 8, 3)
    bnn_hip.set_math("f32")
    net = _bnn(dev, dims, 32, 5)
    rs = np.random.RandomState(6)
    X = rs.uniform(0, 1, (N, 1, 1, dims[0])).astype(np.float32)
    pool = active.ActivePool(epoch.DeviceDataset(X, np.zeros(N, np.int64), device=dev), [0])
    bnn_hip.manual_seed(SEED, counter=400)
    jp = pool.joint_probs(net, S, rows_per_call=32)
    assert state.counter == 400 + S and jp.first_sample == 400
    assert tuple(jp.probs.shape) == (S, N, 3) and jp.probs.dtype == torch.float32 and jp.cond.dtype == jp.marg.dtype == torch.float64
    bnn_hip.manual_seed(SEED, counter=400)
    with torch.no_grad():
        want = torch.softmax(net.forward_mc(torch.from_numpy(X).to(dev), S), dim=-1).cpu().numpy()
        other = torch.softmax(net.forward_mc(torch.from_numpy(X).to(dev), S), dim=-1).cpu().numpy()      # the NEXT S draws
    P = jp.probs.cpu().numpy()
    print(f"shared draws: largest difference {np.abs(P - want).max():.3e}; the next draws differ by {np.abs(P - other).max():.3e}")
    np.testing.assert_allclose(P, want, rtol=0, atol=1e-3)
    assert np.abs(P - other).max() > 1e-2                                     # the comparison can tell draws apart
    np.testing.assert_allclose(P.sum(axis=2), 1.0, atol=1e-6)
    cond, marg = R.entropies(P)
    np.testing.assert_allclose(jp.cond.cpu().numpy(), cond, rtol=0, atol=1e-13)
    np.testing.assert_allclose(jp.marg.cpu().numpy(), marg, rtol=0, atol=1e-13)
    # step 1 through the entries: begin + joint with M = 1
    f64 = dict(dtype=torch.float64, device=dev)
    phat = [torch.empty((1, S), dtype=torch.float32, device=dev) for _ in range(2)]
    expo = [torch.empty(1, dtype=torch.int32, device=dev) for _ in range(2)]
    w, o, base, sc64 = torch.empty(1, **f64), torch.empty(1, **f64), torch.empty(1, **f64), torch.empty(N, **f64)
    sc = torch.empty(N, dtype=torch.float32, device=dev)
    ops.batchbald_begin(ops.batchbald_state_args(probs=jp.probs, cond=jp.cond, labelled=pool._labelled, n_labelled=pool.n_labelled_word,
                                                 phat_in=phat[1], expo_in=expo[1], phat_out=phat[0], expo_out=expo[0], weight=w,
                                                 offset=o, base=base, max_configs=8))
    ops.batchbald_joint(ops.batchbald_joint_args(probs=jp.probs, phat=phat[0], weight=w, offset=o, cond=jp.cond, base=base, scores=sc,
                                                 scores64=sc64, n_configs=1))
    got, bnd = sc64.cpu().numpy(), R.bound(S, marg)
    assert (np.abs(got - (marg - cond)) <= bnd).all()
    mi = ops.mc_predictive(torch.log(jp.probs.clamp_min(1e-30)), "classification").mutual_information.reshape(-1).cpu().numpy()
    print(f"step 1 against F3's mutual_information: largest difference {np.abs(got - mi).max():.3e}, bound {bnd.min():.3e}; "
          f"scores up to {got.max():.3e}")
    assert (np.abs(np.maximum(got, 0.0) - mi) <= bnd).all()
    assert got.max() > 1e-3


# ---------------------------------------------------------------------------------------------------- 5. the learner
def test_learner_rounds_with_batchbald_do_not_synchronise(dev, tmp_path):
    """Two prepared rounds of ActiveLearner(acquisition="batchbald") on a 64-row pool, k = 3, under
    torch.cuda.set_sync_debug_mode("error") (as the F10 rounds test: no timing): the selections are distinct candidates, they
    leave the pool and join the labelled list in the order chosen."""
    from bnn_hip import tasks
    N, B, k = 64, 8, 3
    rs = np.random.RandomState(4)
    X, Y = rs.uniform(0, 1, (N, 1, 1, 16)).astype(np.float32), rs.randint(0, 4, N).astype(np.int64)
    bnn_hip.manual_seed(SEED, counter=10)
    torch.manual_seed(3)
    params = dict(lr=1e-3, hidden_units=32, mode="classification", batch_size=B, num_batches=4, train_samples=2, test_samples=4,
                  x_shape=16, classes=4, mu_init=[-0.2, 0.2], rho_init=[-5, -4], prior_init=[1.0], mixture_prior=False,
                  local_reparam=False, dropout=False, save_dir=str(tmp_path / "m"), epochs=1)
    t = tasks.BNN_Classification("bnn", params)
    initial = list(range(0, 32, 2))
    pool = active.ActivePool(epoch.DeviceDataset(X, Y, device=dev), initial)
    lrn = active.ActiveLearner(t, pool, k, acquisition="batchbald", max_configs=64, seed=5)     # 4, 16, 64 configurations: exact
    first = lrn.round()                                      # warm-up: the step's capture, first launches, the buffers
    lrn.prepare(2)
    torch.cuda.synchronize()
    c0 = state.counter
    torch.cuda.set_sync_debug_mode("error")
    try:
        rest = lrn.run(2)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert pool.n_labelled == 16 + 3 * k == int(pool.n_labelled_word.item()) and pool.round == 3
    assert state.counter - c0 >= 2 * 4                        # each round took its S shared draws (and the training steps theirs)
    picked = torch.cat([first] + rest).cpu().numpy()
    assert picked.dtype == np.int32 and len(set(picked.tolist())) == 3 * k and (picked >= 0).all() and (picked < N).all()
    assert not set(picked.tolist()) & set(initial)
    assert np.array_equal(pool.labelled[-3 * k:].cpu().numpy(), picked)
    assert not pool.candidate[pool.labelled.long()].any() and int(pool.candidate.sum()) == N - pool.n_labelled
