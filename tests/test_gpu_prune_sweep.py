"""The F9 pruning sweep on an MI355X (posthoc.snr_thresholds, posthoc.PruneSweep; bnn_snr_select, bnn_prune_codes,
bnn_pruned_fwd, bnn_prune_sweep_tail): thresholds and masks bit for bit against today's path (snr_threshold,
prune_weights on a copy), the forward and the evaluation against the fp64 restatement of tests/test_prune_sweep_cpu.py,
the loader forms, no model copy and no host synchronisation; the level masks and the compressed network's keep pattern
against the masks the REAL weight_pruning.py left (tests/golden/posthoc.npz, group G11)."""
import copy
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bnn_hip
from bnn_hip import epoch, ops, posthoc, synth
import posthoc_cases as C
from oracle import bnn_oracle as O
from test_prune_sweep_cpu import PAPER_LEVELS, codes_ref, masked_forward_ref, thresholds_ref

FWD_TOL = {"f32": 1e-5, "bf16": 2e-3}          # of the output scale: the bounds of tests/test_gpu_dense_train.py
F32_RTOL = 2e-5                                 # tests/test_gpu_parity.py
LEVELS7 = (0, .25, .5, .75, .95, .98, 1)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _math_back():
    yield
    bnn_hip.set_math("bf16")


def _net(dims, lr, mode, dev):
    import networks
    mp = dict(input_shape=dims[0], classes=dims[2], batch_size=128, hidden_units=dims[1], mode=mode, mu_init=[-0.2, 0.2],
              rho_init=[-5, -4], prior_init=[1.0], mixture_prior=False, local_reparam=lr)
    net = networks.BayesianNetwork(mp)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(*dims, lr).items()})
    return net.to(dev).eval()


def _levels(P):
    """P drop fractions, out of order, with 0 and 1 among them once P allows."""
    base = [.5, 0., .98, .75, .95, 1., .25, .9, .1, .6, .99]
    return tuple(base[:P]) if P > 1 else (.5,)


def _restate(net, ps):
    """The sweep restated from the device's fp32 SNRs: thresholds (caller's order), per layer (W, b, wcode, bcode) in the
    canonical [out, in] layout as float64 / uint8, the survivors per level, and the rank of each level's threshold."""
    lr = bool(net.local_reparam)
    snr, params = [], []
    for l in (net.l1, net.l2, net.l3):
        sw, sb = ops.snr_db(l.weight_mu.detach(), l.weight_rho.detach()).cpu().numpy(), ops.snr_db(l.bias_mu.detach(), l.bias_rho.detach()).cpu().numpy()
        snr.append((sw, sb))
        params.append((l.weight_mu.detach().cpu().numpy(), l.bias_mu.detach().cpu().numpy()))
    thr = thresholds_ref(np.concatenate([a.ravel() for pair in snr for a in pair]), ps)
    order = sorted(range(len(ps)), key=lambda i: ps[i])
    rank = [0] * len(ps)
    for j, i in enumerate(order):
        rank[i] = j
    asc = thr[order]
    layers = []
    for (sw, sb), (w, b) in zip(snr, params):
        wc, bc = codes_ref(sw, asc), codes_ref(sb, asc)
        if lr:
            w, wc = w.T, wc.T
        layers.append((w.astype(np.float64), b.astype(np.float64), wc, bc))
    kept = [sum(int((wc > rank[i]).sum()) + int((bc > rank[i]).sum()) for _, _, wc, bc in layers) for i in range(len(ps))]
    return thr, layers, kept, rank


# ------------------------------------------------------------------------------------------------- 1. thresholds, exact
def _snr_case(n, kind, seed):
    rs = np.random.RandomState(seed)
    v = (rs.standard_normal(n) * 12 + 5).astype(np.float32)
    if kind == "ties":
        v = np.round(v / 8).astype(np.float32) * 8                   # a dozen distinct values
    if kind == "inf" and n > 2:
        v[rs.randint(0, n, max(1, n // 5))] = -np.inf                # mu = 0
    return v


@pytest.mark.parametrize("n", [1, 2, 190, 4097, 2395210])
@pytest.mark.parametrize("kind", ["plain", "ties", "inf"])
def test_thresholds_equal_the_sorted_path_bit_for_bit(dev, n, kind):
    v = torch.from_numpy(_snr_case(n, kind, n % 1000 + len(kind))).to(dev)
    got = posthoc.snr_thresholds(v, LEVELS7)
    assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == (7,)
    want = np.asarray([posthoc.snr_threshold(v, p) for p in LEVELS7], dtype=np.float64)
    np.testing.assert_array_equal(got.cpu().numpy(), want)           # == (NaN where the sorted path gives NaN: -inf + inf)
    np.testing.assert_array_equal(got.cpu().numpy(), thresholds_ref(v.cpu().numpy(), LEVELS7))
    again = posthoc.snr_thresholds(v, LEVELS7)
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))       # bitwise reproducible
    cuts = sorted({0, n // 3, n // 2, n - n // 7, n})                # the same values as segments: never concatenated
    segs = [v[a:b] for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
    seg = posthoc.snr_thresholds(segs, LEVELS7)
    assert torch.equal(got.view(torch.int64), seg.view(torch.int64))
    rev = posthoc.snr_thresholds(v, LEVELS7[::-1])                   # any order in, the same order out
    assert torch.equal(rev.view(torch.int64), got.flip(0).view(torch.int64))


def test_thresholds_order_nans_last(dev):
    v = _snr_case(4097, "plain", 1)
    v[::9] = np.nan
    t = torch.from_numpy(v).to(dev)
    np.testing.assert_array_equal(posthoc.snr_thresholds(t, (0., .5, .8, 1.)).cpu().numpy(),
                                  np.asarray([posthoc.snr_threshold(t, p) for p in (0., .5, .8, 1.)]))


@pytest.mark.parametrize("lr", [False, True])
def test_model_thresholds_equal_the_concatenated_vector(dev, lr):
    net = _net((784, 1200, 10), lr, "classification", dev)
    snrs = posthoc.compute_snr(net)
    assert snrs.numel() == 2395210
    got = posthoc.snr_thresholds(net, LEVELS7).cpu().numpy()
    np.testing.assert_array_equal(got, np.asarray([posthoc.snr_threshold(snrs, p) for p in LEVELS7]))


# ------------------------------------------------------------------------------------------------- 2. masks, exact
@pytest.mark.parametrize("lr", [False, True])
def test_level_codes_equal_prune_weights_on_a_copy(dev, lr):
    net = _net((784, 1200, 10), lr, "classification", dev)
    with torch.no_grad():
        net.l1.weight_mu.view(-1)[7::1001] = 0.0                     # -inf dB: pruned at every level
        net.l3.bias_mu[3] = 0.0
    before = {k: v.clone() for k, v in net.state_dict().items()}
    ps = (.5, 0., .98, .75, .95, 1., .25)
    sweep = posthoc.PruneSweep(net, ps)
    after = net.state_dict()
    assert all(torch.equal(before[k].view(torch.int32), after[k].view(torch.int32)) for k in before)   # bit-identical
    assert sweep.total_parameters == 2395210
    kept = sweep.kept.cpu().numpy()
    thr = sweep.thresholds.cpu().numpy()
    codes = sweep.codes()
    for i, p in enumerate(ps):
        c = copy.deepcopy(net)
        t = posthoc.prune_weights(c, None, p)
        np.testing.assert_array_equal(thr[i], np.float64(t))
        count = 0
        for (wc, bc), l in zip(codes, (c.l1, c.l2, c.l3)):
            wm = l.weight_mu.detach().T if lr else l.weight_mu.detach()
            assert torch.equal(wc > sweep.level_rank[i], wm != 0) and torch.equal(bc > sweep.level_rank[i], l.bias_mu.detach() != 0)
            count += int((wm != 0).sum()) + int((l.bias_mu != 0).sum())
        assert int(kept[i]) == count, (p, kept[i], count)
    # level 0 is not the unpruned network: the threshold is the minimum SNR and the comparison is strict
    zeros = int((before["l1.weight_mu"] == 0).sum()) + 1
    assert kept[1] == 2395210 - zeros and thr[1] == -np.inf and kept[5] == 0
    rthr, layers, rkept, rank = _restate(net, ps)                    # the restatement the forward tests use
    np.testing.assert_array_equal(thr, rthr)
    assert list(kept) == rkept and tuple(rank) == sweep.level_rank
    for (wc, bc), (_, _, rwc, rbc) in zip(codes, layers):
        assert np.array_equal(wc.cpu().numpy(), rwc) and np.array_equal(bc.cpu().numpy(), rbc)


# ------------------------------------------------------------------------------------------------- 3. forward
SHAPES = [((784, 1200, 10), 128, "classification"), ((1, 400, 1), 37, "regression"), ((119, 100, 1), 37, "regression")]


@pytest.mark.parametrize("math_mode", ["f32", "bf16"])
@pytest.mark.parametrize("lr", [False, True])
@pytest.mark.parametrize("dims,rows,mode", SHAPES)
def test_forward_against_the_fp64_masked_forward(dev, dims, rows, mode, lr, math_mode):
    bnn_hip.set_math(math_mode)
    net = _net(dims, lr, mode, dev)
    x_np, _ = synth.synth_batch(mode, rows, dims[0], dims[2], seed=77)
    x = torch.from_numpy(x_np).to(dev)
    tol = FWD_TOL[math_mode]
    for P in (1, 5, 8, 11):
        ps = _levels(P)
        sweep = posthoc.PruneSweep(net, ps)
        got = sweep.forward(x)
        assert tuple(got.shape) == (P, rows, dims[2]) and got.dtype == torch.float32
        _, layers, _, rank = _restate(net, ps)
        g = got.double().cpu().numpy()
        for i, p in enumerate(ps):
            ref = masked_forward_ref(x_np, layers, rank[i], bf16=math_mode == "bf16")
            scale = max(np.abs(ref).max(), 1e-30)
            err = np.abs(g[i] - ref).max()
            print(f"forward {dims} lr={lr} {math_mode} P={P} p={p}: err {err:.3e} scale {scale:.3e}")
            assert err <= tol * scale, (P, p, err, scale)
            if p == 1.:
                assert not g[i].any()                                 # nothing survives: the logits are exactly 0
            if P == 5:                                               # today's path: prune a copy, run it in eval mode
                c = copy.deepcopy(net)
                posthoc.prune_weights(c, None, p)
                with torch.no_grad():
                    old = c.eval()(x).double().cpu().numpy()
                assert np.abs(g[i] - old).max() <= tol * max(np.abs(old).max(), scale), (P, p)
    sweep = posthoc.PruneSweep(net, (0.,))                           # level 0 is not the unpruned network: the minimum-SNR
    assert int(sweep.kept.item()) == sweep.total_parameters - 1      # entry goes, as prune_weights(net, None, 0.) removes it


# ------------------------------------------------------------------------------------------------- 4. counts
def _class_data():
    xs, ys = zip(*[synth.synth_batch("classification", 128, 784, 10, seed=40 + i) for i in range(8)])
    return np.concatenate(xs).reshape(1024, 784), np.concatenate(ys)


@pytest.mark.parametrize("math_mode,cap", [("f32", 0.01), ("bf16", 0.06)])
@pytest.mark.parametrize("lr", [False, True])
def test_evaluate_counts_against_the_restatement(dev, lr, math_mode, cap):
    bnn_hip.set_math(math_mode)
    net = _net((784, 1200, 10), lr, "classification", dev)
    X, Y = _class_data()
    ps = PAPER_LEVELS
    thr, layers, kept, rank = _restate(net, ps)
    refs = [masked_forward_ref(X, layers, rank[i], bf16=math_mode == "bf16") for i in range(len(ps))]
    clear = []
    for i, z in enumerate(refs):                                     # the cap, from the restatement alone
        top = np.sort(z, axis=1)
        ok = (top[:, -1] - top[:, -2]) > 2 * FWD_TOL[math_mode] * np.abs(z).max()
        print(f"counts lr={lr} {math_mode} p={ps[i]}: {100 * (1 - ok.mean()):.2f} % of the rows within the margin, "
              f"{len(set(z.argmax(1)))} classes predicted")
        assert 1 - ok.mean() <= cap
        clear.append(ok)
    sweep = posthoc.PruneSweep(net, ps)
    xd, yd = torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev)
    r = sweep.evaluate((xd, yd))
    assert r.total == 1024 and tuple(r.correct.shape) == (5,) and r.correct.dtype == torch.int64
    np.testing.assert_array_equal(r.thresholds.cpu().numpy(), thr)
    assert list(r.kept.cpu().numpy()) == kept
    probs = r.probs.cpu().numpy()
    correct = r.correct.cpu().numpy()
    for i, z in enumerate(refs):
        pred_ref, pred = z.argmax(1), probs[i].argmax(1)
        ok = clear[i]
        assert np.array_equal(pred[ok], pred_ref[ok])
        assert int(correct[i]) == int((pred == Y).sum())             # the count is the count of the sweep's own predictions
        assert int(((pred == Y) & ok).sum()) == int(((pred_ref == Y) & ok).sum())
        np.testing.assert_allclose(probs[i].sum(1), 1.0, rtol=1e-5)
        nll_ref = float((np.log(np.exp(z - z.max(1, keepdims=True)).sum(1)) + z.max(1) - z[np.arange(1024), Y]).sum())
        print(f"nll p={ps[i]}: {r.nll[i]!r} against {nll_ref!r}")
        if math_mode == "f32":
            np.testing.assert_allclose(r.nll[i], nll_ref, rtol=F32_RTOL)
        cnt, cor, conf = posthoc.ECELoss(bin_step=0.1).bins(r.probs[i], yd)
        for a, b in zip(r.bins[i], (cnt, cor, conf)):
            np.testing.assert_array_equal(a, b)
        ece_i, centers, acc = posthoc.ECELoss(bin_step=0.1)(r.probs[i], yd)
        assert r.ece[i] == ece_i
        np.testing.assert_array_equal(r.reliability[i][0], centers)
        np.testing.assert_array_equal(r.reliability[i][1], acc)
    np.testing.assert_array_equal(r.accuracy, correct / 1024.0)
    again = sweep.evaluate((xd, yd))
    assert torch.equal(again.correct, r.correct) and np.array_equal(again.nll.view(np.int64), r.nll.view(np.int64))


def test_regression_sweep_sums_the_squared_error(dev):
    bnn_hip.set_math("f32")
    net = _net((1, 400, 1), False, "regression", dev)
    x_np, y_np = synth.synth_batch("regression", 300, 1, 1, seed=5)
    ps = (.98, .5, 0.)
    r = posthoc.PruneSweep(net, ps).evaluate((torch.from_numpy(x_np).to(dev), torch.from_numpy(y_np).to(dev)), batch_size=128)
    _, layers, _, rank = _restate(net, ps)
    want = [float(((masked_forward_ref(x_np, layers, rank[i]) - y_np) ** 2).sum()) for i in range(3)]
    assert r.total == 300 and r.correct is None and r.nll is None and r.ece is None
    np.testing.assert_allclose(r.sse, want, rtol=F32_RTOL)


# ------------------------------------------------------------------------------------------------- 5. loader forms
@pytest.mark.parametrize("math_mode", ["f32", "bf16"])
def test_loader_and_pair_give_the_same_counts(dev, math_mode):
    bnn_hip.set_math(math_mode)
    net = _net((784, 1200, 10), True, "classification", dev)
    X, Y = _class_data()
    X, Y = X[:1000], Y[:1000]
    sweep = posthoc.PruneSweep(net, PAPER_LEVELS)
    xd, yd = torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev)
    pair = sweep.evaluate((xd, yd))                                  # 7 x 128 rows and a last minibatch of 104
    ds = epoch.DeviceDataset(X.reshape(1000, 1, 28, 28), Y, device=dev)
    flat = sweep.evaluate(epoch.DeviceLoader(ds, 125, shuffle=False, drop_last=False))     # 8 x 125: not a multiple of the tile
    assert pair.total == flat.total == 1000
    assert torch.equal(pair.correct, flat.correct)
    assert torch.equal(pair.probs.view(torch.int32), flat.probs.view(torch.int32))         # row by row the same bits
    shuffled = sweep.evaluate(epoch.DeviceLoader(ds, 125, shuffle=True, drop_last=False, seed=3))
    assert torch.equal(pair.correct, shuffled.correct)
    short = sweep.evaluate(epoch.DeviceLoader(ds, 128, shuffle=False))                     # drop_last: 7 x 128 = 896 rows
    assert short.total == 896
    assert torch.equal(short.correct, sweep.evaluate((xd[:896], yd[:896])).correct)


# ------------------------------------------------------------------------------------------------- 6. no copy, no sync
def test_sweep_needs_no_model_copies_and_no_host_wait(dev):
    """Method for the second half: torch.cuda.set_sync_debug_mode("error"), as the epoch and bandit tests."""
    bnn_hip.set_math("f32")
    net = _net((784, 1200, 10), False, "classification", dev)
    param_bytes = sum(p.numel() * p.element_size() for p in net.parameters())
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    sweep = posthoc.PruneSweep(net, PAPER_LEVELS)
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated() - base
    print(f"sweep state {grown} bytes; one network copy {param_bytes} bytes")
    assert grown < 5 * param_bytes                                   # what the loop's five copies need
    assert grown < param_bytes                                       # one byte + one mu per parameter: under ONE copy
    X, Y = _class_data()
    xd, yd = torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev)
    ld = epoch.DeviceLoader(epoch.DeviceDataset(X.reshape(1024, 1, 28, 28), Y, device=dev), 128, shuffle=True, seed=1)
    warm = sweep.evaluate((xd, yd)), sweep.evaluate(ld)              # allocations, first launches
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        r1 = sweep.evaluate((xd, yd))
        r2 = sweep.evaluate(ld)
        thr = posthoc.snr_thresholds(net, PAPER_LEVELS)
        y = sweep.forward(xd[:128])
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.equal(r1.correct, warm[0].correct) and torch.equal(r2.correct, r1.correct)
    assert torch.equal(thr.view(torch.int64), sweep.thresholds.view(torch.int64)) and tuple(y.shape) == (5, 128, 10)


# ------------------------------------------------------------------------------------------------- 7. recorded masks
@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "posthoc.npz"))


def _fixture_net(fx, name, dev):
    import networks
    dims, lr, sd = C.snr_net(name)
    np.testing.assert_array_equal(C.state_hash(sd), fx[f"G11/{name}/sha256"])
    mp = dict(input_shape=dims[0], classes=dims[2], batch_size=8, hidden_units=dims[1], mode="classification", mu_init=[-0.2, 0.2],
              rho_init=[-5, -4], prior_init=[1.0], mixture_prior=False, local_reparam=lr)
    net = networks.BayesianNetwork(mp)
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    if f"G11/{name}/snr" in fx:
        snr = fx[f"G11/{name}/snr"]
    else:
        with np.errstate(all="ignore"):
            snr = O.compute_snr(C.flat_order(sd, "mu").astype(np.float64), np.log(1 + np.exp(C.flat_order(sd, "rho").astype(np.float64))))
        np.testing.assert_array_equal(C.sha256(snr), fx[f"G11/{name}/snr_sha256"])
    return net.to(dev).eval(), sd, snr, lr


def _check_mask(fx, name, di, keep, kept, snr, label):
    """The band rule of tests/test_gpu_posthoc.py with the device's own threshold: 2 x 3e-5 dB around the recorded one."""
    thr = float(fx[f"G11/{name}/thresholds"][di])
    if f"G11/{name}/keep/{di}" in fx:
        ref_keep = np.unpackbits(fx[f"G11/{name}/keep/{di}"])[:snr.size].astype(bool)
    else:               # local_reparam: the reference left the network unchanged (recorded); here snr > the recorded threshold
        assert int(fx[f"G11/{name}/unchanged"]) == 1
        ref_keep = snr > thr
    out, band = C.band_differs(keep, ref_keep, snr, thr, 2 * C.BAND_DB)
    print(f"{label} {name} drop {C.DROPS[di]}: {band} in the band, {int((keep != ref_keep).sum())} differ, kept {kept}")
    assert band <= 2 * max(1, snr.size // 1000) and out.size == 0, (label, name, C.DROPS[di], out[:8])
    assert kept == int(keep.sum())


@pytest.mark.parametrize("name", ["small", "large", "lr"])
def test_level_masks_match_the_recorded_reference(dev, fx, name):
    net, sd, snr, lr = _fixture_net(fx, name, dev)
    order = (3, 0, 5, 1, 4, 2)                                       # the levels out of order
    sweep = posthoc.PruneSweep(net, [C.DROPS[i] for i in order])
    thr, kept = sweep.thresholds.cpu().numpy(), sweep.kept.cpu().numpy()
    codes = [(wc.cpu().numpy(), bc.cpu().numpy()) for wc, bc in sweep.codes()]
    for j, di in enumerate(order):
        assert abs(thr[j] - float(fx[f"G11/{name}/thresholds"][di])) <= C.BAND_DB
        keep = np.concatenate([np.concatenate([(wc.T if lr else wc).ravel(), bc]) > sweep.level_rank[j] for wc, bc in codes])
        _check_mask(fx, name, di, keep, int(kept[j]), snr, "codes")


@pytest.mark.parametrize("name,drops", [("small", (1, 2, 4)), ("large", (2, 3)), ("lr", (2,))])
def test_compressed_keep_pattern_matches_the_recorded_reference(dev, fx, name, drops):
    net, sd, snr, lr = _fixture_net(fx, name, dev)
    for di in drops:
        cn = posthoc.compress(net, C.DROPS[di])
        dense = {k: v.cpu().numpy() for k, v in cn.to_dense().items()}
        keep = C.flat_order(dense, "rho") != 0                       # no generated rho is 0: a zero rho is a pruned pair
        assert all(dense[k].shape == sd[k].shape for k in sd)
        same = (C.flat_order(dense, "mu") == C.flat_order(sd, "mu")) & (C.flat_order(dense, "rho") == C.flat_order(sd, "rho"))
        assert same[keep].all() and not C.flat_order(dense, "mu")[~keep].any()
        biases = sum(int((dense[f"{l}.bias_rho"] != 0).sum()) for l in C.LAYERS)
        assert sum(cn.nnz) + biases == int(keep.sum())
        _check_mask(fx, name, di, keep, int(keep.sum()), snr, "compress")
