"""Held-out predictive scores on the device (bnn_mc_score, F12): the kernels against the float64 restatement of
tests/score_ref.py, the determinism and accumulation rules, and the Python surface (net.score / score_graph, epoch.score, the
MLP wrappers) end to end.

Tolerance: integer words exact; fp64 sums and per-row values within 1e-10 max(1, |ref|) (the largest case chains about
S C = 2.6e4 fp64 operations of <= 1 ulp each, a relative error near 6e-12).  row_lpd / row_nll are fp32: one fp32 rounding
(2^-24 relative) of the reference on top of that.  Every test asserts from the restatement alone that its seeded input has no
top-2 gap of the mean probabilities under 1e-6 and no conf M / u M within 1e-9 of an (interior) bin edge, so that no case is
left out of an integer comparison."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bnn_hip
from bnn_hip import epoch, ops, synth

import score_ref

BINS = 10
REL = 1e-10


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _f32_math():
    bnn_hip.set_math("f32")
    yield
    bnn_hip.set_math("bf16")
    bnn_hip.manual_seed(2026)


class Replay:
    def __init__(self, arrays):
        self.q = [torch.from_numpy(np.ascontiguousarray(a)) for a in arrays]

    def sample(self, size):
        t = self.q.pop(0)
        assert tuple(t.shape) == tuple(size)
        return t


def build_net(dev, lr, dims, mode, B):
    import networks
    mp = dict(input_shape=dims[0], classes=dims[2], batch_size=B, hidden_units=dims[1], mode=mode, mu_init=[-0.2, 0.2],
              rho_init=[-5, -4], prior_init=[1.0], mixture_prior=False, local_reparam=lr)
    net = networks.BayesianNetwork(mp)
    sd = synth.synth_state_dict(dims[0], dims[1], dims[2], lr)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net.to(dev).eval()


def install_eps(net, B, S, lr):
    shapes = []
    for l in (net.l1, net.l2, net.l3):
        shapes += [(B, l.weight_mu.shape[1]) if lr else tuple(l.weight_mu.shape), tuple(l.bias_mu.shape)]
    per = [synth.synth_eps(shapes, s) for s in range(S)]
    for li, l in enumerate((net.l1, net.l2, net.l3)):
        if lr:
            l.normal = Replay([a for s in range(S) for a in (per[s][2 * li], per[s][2 * li + 1])])
        else:
            l.weight.normal = Replay([per[s][2 * li] for s in range(S)])
            l.bias.normal = Replay([per[s][2 * li + 1] for s in range(S)])


def words(scores):
    return scores.record.cpu().numpy()


def check_margins(ref, classification=True):
    if classification:
        assert ref["min_top2_gap"] >= 1e-6, ref["min_top2_gap"]
    assert ref["min_edge_distance"] >= 1e-9, ref["min_edge_distance"]


def close_rows(got, want, what):
    """fp32 outputs: one fp32 rounding of the reference on top of the fp64 tolerance."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    tol = 2.0 ** -24 * np.abs(want) + REL * np.maximum(1.0, np.abs(want))
    assert (np.abs(got - want) <= tol).all(), (what, float(np.abs(got - want).max()))


# ----------------------------------------------------------------------------------------------------- classification kernel
CLASS_SHAPES = [(1, 1, 128, 10), (1, 10, 128, 10), (1, 64, 7, 3), (1, 5, 33, 100), (1, 257, 4, 2), (3, 10, 128, 10)]


def class_case(shape):
    """(logits, labels, n_valid).  (1, 10, 128, 10) carries four rows whose label has logit -80 against two classes near +80:
    an fp32 softmax gives p_y = 0 there.  (3, 10, 128, 10) is ragged: its last 37 rows are padding -- NaN logits, label -1."""
    G, S, B, C = shape
    rng = np.random.default_rng(G * 1000 + S * 7 + C)
    lg = (rng.standard_normal((G, S, B, C)) * 3).astype(np.float32)
    y = rng.integers(0, C, size=(G, B)).astype(np.int64)
    n_valid = G * B
    if shape == (1, 10, 128, 10):
        lg[0, :, :4, 2:] = (-80.0 + rng.standard_normal((S, 4, C - 2))).astype(np.float32)
        lg[0, :, :4, :2] = (80.0 + rng.standard_normal((S, 4, 2))).astype(np.float32)
        y[0, :4] = 2
    if G == 3:
        n_valid = G * B - 37
        flat = lg.transpose(0, 2, 1, 3).reshape(G * B, S, C).copy()
        flat[n_valid:] = np.nan
        lg = np.ascontiguousarray(flat.reshape(G, B, S, C).transpose(0, 2, 1, 3))
        y.reshape(-1)[n_valid:] = -1
    return lg, y, n_valid


@pytest.mark.parametrize("shape", CLASS_SHAPES)
def test_classification_kernel_matches_float64(dev, shape):
    G, S, B, C = shape
    lg, y, n_valid = class_case(shape)
    ref = score_ref.classification(lg, y, BINS, n_valid)
    check_margins(ref)
    sc = ops.mc_score(torch.from_numpy(lg).to(dev), torch.from_numpy(y).to(dev), "classification", bins=BINS, n_valid=n_valid,
                      rows=True)
    torch.cuda.synchronize()
    got = words(sc)
    print(shape, "record", got[:2], got.view(np.float64)[2:5], "ref", ref["sum_lpd"], ref["sum_nll"], ref["sum_brier"])
    assert np.isfinite(got.view(np.float64)[2:5]).all()
    score_ref.assert_record(got, ref, "classification", BINS, REL)
    close_rows(sc.row_lpd.cpu().numpy().reshape(-1)[:n_valid], ref["lpd"], "row_lpd")
    close_rows(sc.row_nll.cpu().numpy().reshape(-1)[:n_valid], ref["nll"], "row_nll")
    r = sc.read()
    assert r.n == n_valid and r.bin_count.sum() == n_valid
    if shape == (1, 10, 128, 10):                                           # the underflow rows: finite where fp32 gives -inf
        p32 = torch.softmax(torch.from_numpy(lg[0, :, :4]), -1)[..., 2]
        assert float(p32.max()) == 0.0
        assert np.isfinite(sc.row_lpd.cpu().numpy()[0, :4]).all() and (ref["lpd"][:4] < -100).all()


def test_padding_rows_are_left_unwritten(dev):
    lg, y, n_valid = class_case((3, 10, 128, 10))
    sc = ops.Scores("classification", BINS, dev)
    sc.row_lpd = torch.full((3, 128), 7.0, device=dev)
    sc.row_nll = torch.full((3, 128), 7.0, device=dev)
    sc.accumulate(torch.from_numpy(lg).to(dev), torch.from_numpy(y).to(dev), n_valid=n_valid, rows=True)
    torch.cuda.synchronize()
    assert (sc.row_lpd.reshape(-1)[n_valid:] == 7.0).all() and (sc.row_nll.reshape(-1)[n_valid:] == 7.0).all()
    assert (sc.row_lpd.reshape(-1)[:n_valid] != 7.0).all()


def test_a_nan_logit_in_a_valid_row_shows_in_the_sums_and_not_in_the_bins(dev):
    shape = (1, 64, 7, 3)
    lg, y, _ = class_case(shape)
    lg[0, 5, 3, 1] = np.nan
    ref = score_ref.classification(lg, y, BINS)
    check_margins(ref)
    sc = ops.mc_score(torch.from_numpy(lg).to(dev), torch.from_numpy(y).to(dev), "classification", bins=BINS)
    torch.cuda.synchronize()
    got = words(sc)
    assert got[0] == 7 and np.isnan(got.view(np.float64)[2:5]).all()
    assert got[8::3].sum() == 6
    score_ref.assert_record(got, ref, "classification", BINS, REL)


def test_a_label_outside_the_classes_gives_minus_infinity(dev):
    lg, y, _ = class_case((1, 5, 33, 100))
    y[0, 7], y[0, 8] = 100, -5
    ref = score_ref.classification(lg, y, BINS)
    sc = ops.mc_score(torch.from_numpy(lg).to(dev), torch.from_numpy(y).to(dev), "classification", bins=BINS, rows=True)
    torch.cuda.synchronize()
    assert (sc.row_lpd.cpu().numpy()[0, 7:9] == -np.inf).all() and (sc.row_nll.cpu().numpy()[0, 7:9] == np.inf).all()
    score_ref.assert_record(words(sc), ref, "classification", BINS, REL)


# ----------------------------------------------------------------------------------------------------- regression kernel
REG_SHAPES = [(1, 10, 400, 1), (1, 1, 128, 1), (2, 33, 65, 3), (1, 1024, 8, 1)]


def reg_case(shape, sigma):
    """(outputs, targets, n_valid): samples and targets within a few sigma of a common centre, so that the PIT takes values
    across [0, 1].  (1, 10, 400, 1): targets 0 and 1 sit 50 sigma above / below every sample.  (2, 33, 65, 3) is ragged."""
    G, S, B, C = shape
    rng = np.random.default_rng(S * 13 + B + int(sigma * 10))
    centre = rng.standard_normal((G, 1, B, C))
    f = (centre + 1.5 * sigma * rng.standard_normal((G, S, B, C))).astype(np.float32)
    t = (centre[:, 0] + 1.5 * sigma * rng.standard_normal((G, B, C))).astype(np.float32)
    n_valid = G * B
    if shape == (1, 10, 400, 1):
        t[0, 0, 0] = f[0, :, 0, 0].max() + np.float32(50 * sigma)
        t[0, 1, 0] = f[0, :, 1, 0].min() - np.float32(50 * sigma)
    if G == 2:
        n_valid = G * B - 21
        f[1, :, B - 21:] = np.nan
        t[1, B - 21:] = np.nan
    return f, t, n_valid


@pytest.mark.parametrize("sigma", [0.1, 1.0])
@pytest.mark.parametrize("shape", REG_SHAPES)
def test_regression_kernel_matches_float64(dev, shape, sigma):
    G, S, B, C = shape
    f, t, n_valid = reg_case(shape, sigma)
    ref = score_ref.regression(f, t, sigma, BINS, n_valid)
    check_margins(ref, classification=False)
    sc = ops.mc_score(torch.from_numpy(f).to(dev), torch.from_numpy(t).to(dev), "regression", sigma=sigma, bins=BINS,
                      n_valid=n_valid, rows=True)
    torch.cuda.synchronize()
    got = words(sc)
    print(shape, sigma, "record", got[:2], got.view(np.float64)[2:6], "ref", ref["sum_lpd"], ref["sum_nll"], ref["sum_sq"], ref["sum_abs"])
    assert np.isfinite(got.view(np.float64)[2:6]).all()
    score_ref.assert_record(got, ref, "regression", BINS, REL)
    close_rows(sc.row_lpd.cpu().numpy().reshape(-1)[:n_valid], ref["row_lpd"], "row_lpd")
    close_rows(sc.row_nll.cpu().numpy().reshape(-1)[:n_valid], ref["row_nll"], "row_nll")
    r = sc.read()
    assert r.n == n_valid * C and r.rows == n_valid and r.pit.sum() == n_valid * C
    np.testing.assert_allclose(r.coverage(1.0), 1.0)
    if shape == (1, 10, 400, 1):                                            # 50 sigma away: finite density, outer PIT bins
        assert np.isfinite(sc.row_lpd.cpu().numpy()[0, :2]).all() and (ref["lpd"][:2] < -1000).all()
        assert ref["bin"][0] == BINS - 1 and ref["bin"][1] == 0


# ----------------------------------------------------------------------------------------------------- determinism, accumulation
@pytest.mark.parametrize("mode", ["classification", "regression"])
def test_the_same_call_twice_is_bit_identical_and_halves_accumulate_to_the_whole(dev, mode):
    if mode == "classification":
        lg, y, _ = class_case((3, 10, 128, 10))
        lg, y = np.nan_to_num(lg[:2], nan=0.5), np.abs(y[:2])               # two whole groups, no padding
        kw = {}
    else:
        lg, y, _ = reg_case((2, 33, 65, 3), 0.1)
        lg, y = np.nan_to_num(lg, nan=0.25), np.nan_to_num(y, nan=0.3)
        kw = dict(sigma=0.1)
    L, Y = torch.from_numpy(lg).to(dev), torch.from_numpy(y).to(dev)
    a = ops.mc_score(L, Y, mode, bins=BINS, **kw)
    b = ops.mc_score(L, Y, mode, bins=BINS, **kw)
    again = a.record.clone()
    ops.Scores.accumulate(a, L, Y, overwrite=True, **kw)                   # the same record written a second time
    torch.cuda.synchronize()
    assert torch.equal(a.record, b.record) and torch.equal(a.record, again)
    halves = ops.Scores(mode, BINS, dev)
    for g in range(2):
        ops.mc_score(L[g:g + 1].contiguous(), Y[g:g + 1].contiguous(), mode, bins=BINS, record=halves, **kw)
    torch.cuda.synchronize()
    w, h = words(a), words(halves)
    ii, ff = score_ref.INT_WORDS(BINS), score_ref.F64_WORDS(BINS)
    assert np.array_equal(w[ii], h[ii]) and w[0] == 2 * lg.shape[2]
    wf, hf = w.view(np.float64)[ff], h.view(np.float64)[ff]
    assert (np.abs(wf - hf) <= 1e-12 * np.abs(wf)).all(), (wf, hf)
    halves.reset()
    torch.cuda.synchronize()
    assert not words(halves).any()


# ----------------------------------------------------------------------------------------------------- the Python surface
@pytest.mark.parametrize("lr,mode,dims", [(False, "classification", (20, 16, 3)), (True, "regression", (1, 16, 1))])
def test_net_score_equals_the_restatement_of_forward_mc_under_the_same_epsilon(dev, lr, mode, dims):
    B, S, sigma = 8, 4, 0.1
    net = build_net(dev, lr, dims, mode, B)
    x, y = synth.synth_batch(mode, B, dims[0], dims[2])
    x = torch.from_numpy(np.asarray(x, np.float32).reshape(B, dims[0])).to(dev)
    install_eps(net, B, S, lr)
    logits = net.forward_mc(x, S).cpu().numpy()[None]
    if mode == "classification":
        ref = score_ref.classification(logits, y[None], BINS)
    else:
        ref = score_ref.regression(logits, y[None], sigma, BINS)
    check_margins(ref, mode == "classification")
    install_eps(net, B, S, lr)
    sc = net.score(x, torch.from_numpy(y).to(dev), S, sigma=sigma, bins=BINS)
    torch.cuda.synchronize()
    score_ref.assert_record(words(sc), ref, mode, BINS, REL)
    r = sc.read()
    assert r.n == B * (1 if mode == "classification" else dims[2])
    np.testing.assert_allclose(r.lpd, ref["sum_lpd"] / r.n, rtol=1e-9)


def _dataset(dev, N, d, C, seed=5):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0, 1, (N, d)).astype(np.float32)
    y = rng.integers(0, C, N).astype(np.int64)
    return epoch.DeviceDataset(torch.from_numpy(x), torch.from_numpy(y), device=dev)


def test_epoch_score_covers_a_ragged_data_set_at_the_loops_sample_indices(dev):
    """300 rows at B = 128, drop_last=False (44 real rows in the last minibatch), chunk = 2: the record equals ops.mc_score
    folded over the stacked evaluation's logits from the same counter, and the counter ends where ActivePool.score leaves it."""
    N, B, S, SEED, k, chunk = 300, 128, 4, 20271, 900, 2
    net = build_net(dev, False, (20, 16, 3), "classification", B)
    ds = _dataset(dev, N, 20, 3)
    loader = epoch.EvalLoader(ds, B, drop_last=False)
    assert len(loader) == 3
    bnn_hip.manual_seed(SEED, counter=k)
    sc = epoch.score(net, loader, S, bins=BINS, chunk=chunk)
    end = bnn_hip.runtime.state.counter
    torch.cuda.synchronize()
    got = words(sc)
    assert got[0] == 300 and sc.read().n == 300

    bnn_hip.manual_seed(SEED, counter=k)
    want = ops.Scores("classification", BINS, dev)
    for g0 in range(0, 3, chunk):
        G = min(chunk, 3 - g0)
        a, b = g0 * B, min(N, (g0 + G) * B)
        xs = torch.zeros((G * B, 20), device=dev)
        xs[:b - a] = ds.x[a:b]
        ys = torch.zeros(G * B, dtype=torch.int64, device=dev)
        ys[:b - a] = ds.y[a:b]
        ev = net.predictive_graph(xs.view(G, B, 20), S, stacked=True, capture=False)
        ev.replay()
        ops.mc_score(ev.logits, ys.view(G, B), "classification", bins=BINS, groups=G, n_valid=b - a, record=want)
    torch.cuda.synchronize()
    assert bnn_hip.runtime.state.counter == end == k + 3 * S
    assert np.array_equal(got, words(want))

    pool = bnn_hip.ActivePool(ds, [0])
    bnn_hip.manual_seed(SEED, counter=k)
    pool.score(net, S, "bald", chunk)
    assert bnn_hip.runtime.state.counter == end
    short = epoch.score(net, epoch.DeviceLoader(ds, B, shuffle=False), S, bins=BINS)      # drop_last: 2 x 128 rows
    torch.cuda.synchronize()
    assert words(short)[0] == 256


def test_score_graph_accumulates_over_replays_with_fresh_epsilon(dev):
    B, S = 8, 4
    net = build_net(dev, False, (20, 16, 3), "classification", B)
    x, y = synth.synth_batch("classification", B, 20, 3)
    x = torch.from_numpy(np.asarray(x, np.float32).reshape(B, 20)).to(dev)
    y = torch.from_numpy(y).to(dev)
    for capture in (True, "calls", False):
        g = net.score_graph(x, y, S, bins=BINS, capture=capture)
        assert tuple(g.x.shape) == (B, 20) and tuple(g.y.shape) == (B,) and g.y.dtype == torch.int64
        torch.cuda.synchronize()
        assert not words(g.scores).any()                                    # construction leaves the record as it found it
        first = None
        for i in range(3):
            g.replay()
            if i == 0:
                first = g.scores.record.clone()
        torch.cuda.synchronize()
        w = words(g.scores)
        assert w[0] == 3 * B and w[8::3].sum() == 3 * B, capture
        assert w.view(np.float64)[2] != 3 * first.cpu().numpy().view(np.float64)[2]      # fresh epsilon per replay
        assert g.scores.read().n == 3 * B


@pytest.mark.parametrize("mode", ["classification", "regression"])
def test_mlp_wrappers_score_their_own_outputs(dev, mode):
    import networks
    B, S, sigma, seed, c = 16, 5, 0.5, 20272, 40
    inp, out = (16, 3) if mode == "classification" else (4, 2)
    torch.manual_seed(3)
    params = dict(input_shape=inp, classes=out, batch_size=B, hidden_units=32, mode=mode)
    g = torch.Generator().manual_seed(4)
    x = (torch.rand((B, 1, 4, 4), generator=g) if mode == "classification" else torch.randn((B, inp), generator=g)).to(dev)
    y = (torch.randint(0, out, (B,), generator=g) if mode == "classification" else torch.randn((B, out), generator=g)).to(dev)

    def ref_of(logits):
        lg = logits.detach().cpu().numpy()[None]
        if mode == "classification":
            return score_ref.classification(lg, y.cpu().numpy()[None], BINS)
        return score_ref.regression(lg, y.cpu().numpy()[None], sigma, BINS)

    drop = networks.MLP_Dropout(params).to(dev)
    bnn_hip.manual_seed(seed, counter=c)
    logits = drop.mc_forward(x, S)
    bnn_hip.manual_seed(seed, counter=c)
    sc = drop.score(x, y, S, sigma=sigma, bins=BINS)
    torch.cuda.synchronize()
    ref = ref_of(logits)
    check_margins(ref, mode == "classification")
    score_ref.assert_record(words(sc), ref, mode, BINS, REL)

    plain = networks.MLP(params).to(dev).eval()
    with torch.no_grad():
        out1 = plain(x).float()
    sc = plain.score(x, y, sigma=sigma, bins=BINS)
    torch.cuda.synchronize()
    ref = ref_of(out1[None])
    check_margins(ref, mode == "classification")
    score_ref.assert_record(words(sc), ref, mode, BINS, REL)
    np.testing.assert_allclose(ref["lpd"], -ref["nll"], rtol=1e-13, atol=1e-13)      # one sample: lpd = -nll
