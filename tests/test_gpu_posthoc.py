"""F3 / F4 on the GPU: the ECE and SNR-pruning kernels against what the REAL compute_ece.py:14-57 and
weight_pruning.py:85-115 returned (tests/golden/posthoc.npz, recorded by oracle/make_golden_posthoc.py; parity pinned by
that fixture) and against the oracle's restatement of them, itself pinned by the same fixture
(tests/test_posthoc_golden_cpu.py).  The inputs are regenerated from tests/posthoc_cases.py and hash-checked.

Three behaviours differ from the reference ON PURPOSE and are asserted as such, with the recorded
reference result cited: a NaN in the SNR list (reference: every threshold NaN, everything masked; here NaN orders last), a
local_reparam network (reference: returned unchanged; here pruned), and +-inf order statistics (reference: np.percentile
gives NaN from inf - inf; here the order statistic itself)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import posthoc_cases as C
from bnn_hip import ops, posthoc, synth
from oracle import bnn_oracle as O

SNR_TOL_DB = 3e-5                                            # the bound of test_snr_kernel_matches_torch_and_numpy below


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _probs(n, classes, seed, alpha):
    rs = np.random.RandomState(seed)
    p = rs.dirichlet([alpha] * classes, size=n).astype(np.float32)
    labels = np.where(rs.uniform(size=n) < 0.7, p.argmax(1), rs.randint(0, classes, n)).astype(np.int64)
    return p, labels


@pytest.mark.parametrize("n,classes,step,alpha", [(10000, 10, 0.1, 0.3), (1000, 10, 0.1, 0.2), (4097, 3, 0.25, 0.5), (257, 37, 0.1, 0.05)])
def test_ece_kernel_matches_the_reference_restatement(dev, n, classes, step, alpha):
    p, labels = _probs(n, classes, 11 + n, alpha)
    ece_ref, centers_ref, acc_ref, (cnt, cor, conf) = O.ece_reference(p, labels, step, classes)
    crit = posthoc.ECELoss(bin_step=step, num_classes=classes)
    ece, centers, acc = crit(torch.from_numpy(p).to(dev), torch.from_numpy(labels).to(dev))
    c2, r2, m2 = crit.bins(torch.from_numpy(p).to(dev), torch.from_numpy(labels).to(dev))
    np.testing.assert_array_equal(c2, cnt)
    np.testing.assert_array_equal(r2, cor)
    have = cnt > 0
    np.testing.assert_allclose(m2[have], conf[have], rtol=1e-6)
    np.testing.assert_allclose(centers, centers_ref, rtol=0, atol=0)
    np.testing.assert_allclose(acc, acc_ref, rtol=1e-12)
    if have.all():                                         # the reference's own loop is only defined then
        np.testing.assert_allclose(ece, ece_ref, rtol=1e-6)
    else:                                                  # the kernel skips empty bins: the plain definition of ECE
        want = sum(abs(conf[b] - cor[b] / cnt[b]) * cnt[b] / cnt.sum() for b in range(len(cnt)) if cnt[b] > 0)
        np.testing.assert_allclose(ece, want, rtol=1e-6)
    again, _, _ = crit(torch.from_numpy(p).to(dev), torch.from_numpy(labels).to(dev))
    assert again == ece                                    # no float atomics: bitwise reproducible


def test_ece_of_mc_averaged_predictions(dev):
    """The consumer chain of compute_ece.py:62-78: predict (MC-averaged softmax) -> ECE, all on the device."""
    import networks
    torch.manual_seed(0)
    mp = dict(input_shape=784, classes=10, batch_size=128, hidden_units=64, mode="classification", mu_init=[-0.2, 0.2],
              rho_init=[-5, -4], prior_init=[1.0], mixture_prior=False, local_reparam=False)
    net = networks.BayesianNetwork(mp).to(dev).eval()
    xs, ys = zip(*[synth.synth_batch("classification", 128, 784, 10, seed=40 + i) for i in range(4)])
    probs = torch.cat([net.predict_mc(torch.from_numpy(x).to(dev), 5)[1] for x in xs])
    labels = torch.from_numpy(np.concatenate(ys)).to(dev)
    ece, centers, acc = posthoc.ECELoss()(probs, labels)
    ref = O.ece_reference(probs.cpu().numpy(), labels.cpu().numpy())
    cnt = ref[3][0]
    assert 0.0 <= ece <= 1.0 and len(centers) == int((cnt > 0).sum())
    if (cnt > 0).all():
        np.testing.assert_allclose(ece, ref[0], rtol=1e-6)


@pytest.mark.parametrize("shape", [(1200, 784), (37, 5), (4096, 4096)])
def test_snr_kernel_matches_torch_and_numpy(dev, shape):
    rs = np.random.RandomState(5)
    mu = torch.from_numpy(rs.uniform(-0.2, 0.2, shape).astype(np.float32))
    rho = torch.from_numpy(rs.uniform(-5, -4, shape).astype(np.float32))
    mu.view(-1)[3] = 0.0                                    # |mu| = 0: -inf dB, pruned at any threshold
    got = ops.snr_db(mu.to(dev), rho.to(dev)).cpu()
    ref = 10 * torch.log10(torch.abs(mu) / torch.log1p(torch.exp(rho)))          # weight_pruning.py:100
    assert got.view(-1)[3] == -float("inf")
    ok = torch.isfinite(ref)
    np.testing.assert_allclose(got[ok].numpy(), ref[ok].numpy(), rtol=0, atol=3e-5)
    ref64 = O.compute_snr(mu.double().numpy(), np.log(1 + np.exp(rho.double().numpy())))   # :85-87 / :42-43 in numpy
    np.testing.assert_allclose(got[ok].numpy(), ref64[ok.numpy()], rtol=0, atol=3e-5)


@pytest.mark.parametrize("drop", [0.5, 0.25, 0.9])
def test_snr_pruning_of_a_network(dev, drop):
    """posthoc.prune_weights on the drop-in network against the oracle's restatement of weight_pruning.py:89-115 fed
    with the reference's float64 SNR list: same survivors (up to elements within fp32 rounding of the threshold),
    pruned entries left at (0, 0), the state_dict round-trips."""
    import networks
    mp = dict(input_shape=784, classes=10, batch_size=128, hidden_units=1200, mode="classification", mu_init=[-0.2, 0.2],
              rho_init=[-5, -4], prior_init=[1.0], mixture_prior=False, local_reparam=False)
    net = networks.BayesianNetwork(mp)
    sd = synth.synth_state_dict(784, 1200, 10, False)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    layers = [tuple(torch.from_numpy(sd[f"{l}.{n}"]) for n in synth.PARAM_NAMES) for l in synth.LAYER_NAMES]
    # the reference's threshold list: named_parameters() order, python floats, numpy float64 (weight_pruning.py:15-40)
    mus = np.concatenate([sd[f"{l}.{n}"].ravel() for l in synth.LAYER_NAMES for n in ("weight_mu", "bias_mu")]).astype(np.float64)
    rhos = np.concatenate([sd[f"{l}.{n}"].ravel() for l in synth.LAYER_NAMES for n in ("weight_rho", "bias_rho")]).astype(np.float64)
    snrs = O.compute_snr(mus, np.log(1 + np.exp(rhos)))
    want, thr_ref = O.prune_weights(layers, snrs, drop)
    net.to(dev)
    dsnr = posthoc.compute_snr(net)
    assert dsnr.numel() == snrs.size
    np.testing.assert_allclose(np.sort(dsnr.cpu().numpy()), np.sort(snrs), rtol=0, atol=3e-5)
    thr = posthoc.prune_weights(net, None, drop)
    assert abs(thr - thr_ref) <= 3e-5
    got = {k: v.cpu() for k, v in net.state_dict().items()}
    total, differ = 0, 0
    for l, w in zip(synth.LAYER_NAMES, want):
        for n, ref in zip(synth.PARAM_NAMES, w):
            g = got[f"{l}.{n}"]
            total += g.numel()
            differ += int((g != ref).sum())
            if "mu" in n:
                assert bool(((g == 0) == (got[f"{l}.{n.replace('mu', 'rho')}"] == 0)).all())
    assert differ <= 4, differ                               # only elements whose SNR rounds across the threshold
    kept = sum(int((got[f"{l}.{n}"] != 0).sum()) for l in synth.LAYER_NAMES for n in ("weight_mu", "bias_mu"))
    assert abs(kept - (1 - drop) * snrs.size) <= 4
    net.load_state_dict(got)                                  # the 12-key state_dict survives pruning


# =========================================================================================== pinned by tests/golden/posthoc.npz
COMPARED = [n for n, (_, compared, _) in C.ECE_CASES.items() if compared]
RAISING = [n for n, (_, compared, _) in C.ECE_CASES.items() if not compared]


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "posthoc.npz"))


def _ece_inputs(fx, name, dev):
    p, y, step, classes = C.ece_case(name)
    np.testing.assert_array_equal(C.sha256(p, y), fx[f"G10/{name}/sha256"])
    return p, y, step, classes, torch.from_numpy(p).to(dev), torch.from_numpy(y).to(dev)


@pytest.mark.parametrize("name", COMPARED)
def test_ece_kernel_matches_the_recorded_reference(dev, fx, name):
    """Every bin populated, the real ECELoss returned: ece at rtol 1e-6 (this file's bound), the centers and bin_acc =
    corrects / counts exact; counts, corrects and confidence sums against the pinned restatement; bitwise repeatable."""
    p, y, step, classes, pd, yd = _ece_inputs(fx, name, dev)
    crit = posthoc.ECELoss(bin_step=step, num_classes=classes)
    ece, centers, acc = crit(pd, yd)
    c2, r2, m2 = crit.bins(pd, yd)
    print(f"{name}: ece {ece!r} recorded {float(fx[f'G10/{name}/ece'])!r} rel {abs(ece / float(fx[f'G10/{name}/ece']) - 1):.2e}")
    np.testing.assert_allclose(ece, fx[f"G10/{name}/ece"], rtol=1e-6)
    np.testing.assert_array_equal(centers, fx[f"G10/{name}/centers"])
    np.testing.assert_array_equal(acc, r2 / c2)
    np.testing.assert_array_equal(acc, fx[f"G10/{name}/bin_acc"])
    _, _, _, (cnt, cor, conf) = O.ece_reference(p, y, step, classes)
    np.testing.assert_array_equal(c2, cnt)
    np.testing.assert_array_equal(r2, cor)
    np.testing.assert_allclose(m2, conf, rtol=1e-6)
    again = crit(pd, yd)
    assert again[0] == ece and np.array_equal(again[2], acc)
    assert all(np.array_equal(a, b) for a, b in zip(crit.bins(pd, yd), (c2, r2, m2)))


@pytest.mark.parametrize("name", RAISING)
def test_ece_kernel_where_the_reference_raises(dev, fx, name):
    """Recorded for all three (n = 1, the sparse 257 x 37 case, bin_step 0.05): the reference raises IndexError, its loop
    walks off the compressed bin_acc array once a bin is empty.  The kernel returns the plain fp64 definition over the
    non-empty bins."""
    assert str(fx[f"G10/{name}/raised"]) == "IndexError"
    p, y, step, classes, pd, yd = _ece_inputs(fx, name, dev)
    crit = posthoc.ECELoss(bin_step=step, num_classes=classes)
    ece, centers, acc = crit(pd, yd)
    c2, r2, m2 = crit.bins(pd, yd)
    _, centers_ref, acc_ref, (cnt, cor, conf) = O.ece_reference(p, y, step, classes)
    np.testing.assert_array_equal(c2, cnt)
    np.testing.assert_array_equal(r2, cor)
    have = cnt > 0
    assert not have.all()
    np.testing.assert_allclose(m2[have], conf[have], rtol=1e-6)
    np.testing.assert_array_equal(centers, centers_ref)
    np.testing.assert_array_equal(acc, acc_ref)
    want = sum(abs(conf[b] - cor[b] / cnt[b]) * cnt[b] / cnt.sum() for b in range(len(cnt)) if cnt[b] > 0)
    np.testing.assert_allclose(ece, want, rtol=1e-6)
    assert crit(pd, yd)[0] == ece


# ------------------------------------------------------------------------------------------------------------ SNR (G11)
def _device_net(fx, name, dev):
    """The drop-in network loaded with a fixture network's (hash-checked) state; (net, state dict, float64 SNR list)."""
    import networks
    dims, lr, sd = C.snr_net(name)
    np.testing.assert_array_equal(C.state_hash(sd), fx[f"G11/{name}/sha256"])
    mp = dict(input_shape=dims[0], classes=dims[2], batch_size=8, hidden_units=dims[1], mode="classification", mu_init=[-0.2, 0.2],
              rho_init=[-5, -4], prior_init=[1.0], mixture_prior=False, local_reparam=lr)
    net = networks.BayesianNetwork(mp)
    net.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    if f"G11/{name}/snr" in fx:
        snr = fx[f"G11/{name}/snr"]
    else:                                                    # the large network: the list restated, its hash recorded
        with np.errstate(all="ignore"):
            snr = O.compute_snr(C.flat_order(sd, "mu").astype(np.float64), np.log(1 + np.exp(C.flat_order(sd, "rho").astype(np.float64))))
        np.testing.assert_array_equal(C.sha256(snr), fx[f"G11/{name}/snr_sha256"])
    return net.to(dev).eval(), sd, snr


def _bits(fx, name, key, n):
    k = f"G11/{name}/{key}"
    return np.unpackbits(fx[k])[:n].astype(bool) if k in fx else None


def _state(net):
    return {k: v.detach().cpu().numpy() for k, v in net.state_dict().items()}


def _keep(before, after):
    """The survivors in collect_weights order, as the recorder reads them: a pruned pair is (mu * 0, rho * 0), no rho is 0."""
    rb, ra, ma = C.flat_order(before, "rho"), C.flat_order(after, "rho"), C.flat_order(after, "mu")
    return (ra != 0) & ~np.isnan(rb) & ~np.isnan(ma)


def _canon(a):
    """fp32 bits, every NaN as one pattern (the sign and payload of inf * 0 belong to the machine that multiplies);
    signed zeros and everything else bit for bit."""
    a = np.ascontiguousarray(a, np.float32)
    bits = a.view(np.int32).copy()
    bits[np.isnan(a)] = 0x7FC00000
    return bits


def _band12(sd, band):
    """The band mask (collect_weights order) laid out like C.flat12: the same flag for mu and rho of an element."""
    parts, o = {}, 0
    for l in C.LAYERS:
        for kind in ("weight", "bias"):
            t = sd[f"{l}.{kind}_mu"]
            parts[f"{l}.{kind}_mu"] = parts[f"{l}.{kind}_rho"] = band[o:o + t.size].astype(np.float32)
            o += t.size
    return C.flat12(parts) > 0


def _assert_band_rule(fx, name, di, sd, after, snr, width, label):
    """Every element outside the band |recorded float64 SNR - recorded threshold| <= width is what the reference left:
    bit for bit where the fixture stores the tensors, the keep mask and the kept count everywhere."""
    thr = float(fx[f"G11/{name}/thresholds"][di])
    keep, ref_keep = _keep(sd, after), _bits(fx, name, f"keep/{di}", snr.size)
    out, band = C.band_differs(keep, ref_keep, snr, thr, width)
    moved = int((keep != ref_keep).sum())
    print(f"{label} {name} drop {C.DROPS[di]}: {band} in the band, {moved} differ, kept {int(keep.sum())} recorded {int(fx[f'G11/{name}/kept'][di])}")
    assert band <= max(1, snr.size // 1000) * (2 if width > C.BAND_DB else 1)
    assert out.size == 0, (label, name, C.DROPS[di], out[:8], snr[out[:8]], thr)
    assert abs(int(keep.sum()) - int(fx[f"G11/{name}/kept"][di])) <= moved
    key = f"G11/{name}/pruned/{0 if name == 'nan' else di}"
    if key in fx:
        with np.errstate(invalid="ignore"):
            b12 = _band12(sd, np.abs(snr - thr) <= width)
        diff = _canon(C.flat12(after)) != _canon(fx[key])
        assert not (diff & ~b12).any(), (label, name, C.DROPS[di], np.flatnonzero(diff & ~b12)[:8])


@pytest.mark.parametrize("name", ["small", "large", "edges", "nan", "lr"])
def test_snr_db_matches_the_recorded_float64_list(dev, fx, name):
    """Finite entries of the reference's float64 list within 3e-5 dB, the non-finite ones of the same class at the same
    places.  One recorded exception: at rho = 89 the reference's float64 list holds 10 log10(|mu| / 89) while its own
    fp32 torch arithmetic (weight_pruning.py:98-104, the one that makes the masks) has sigma = +inf and SNR = -inf --
    recorded as f32_above_neg_inf; the kernel follows the masks' arithmetic there and must give -inf."""
    net, sd, want = _device_net(fx, name, dev)
    got = posthoc.compute_snr(net).cpu().numpy().astype(np.float64)
    assert got.shape == want.shape
    above = _bits(fx, name, "f32_above_neg_inf", want.size)
    two_paths = np.zeros(want.size, bool) if above is None else np.isfinite(want) & ~above
    assert np.array_equal(two_paths, C.flat_order(sd, "rho") == 89.0)
    assert (got[two_paths] == -np.inf).all()
    rest = ~two_paths
    fin = np.isfinite(want) & rest
    odd = np.flatnonzero(~np.isfinite(want) | ~np.isfinite(got))
    print(f"{name}: non-finite or edge entries (index, recorded, device): {[(int(i), float(want[i]), float(got[i])) for i in odd]}")
    low = np.argsort(np.where(fin, want, np.inf))[:6]
    print(f"{name}: lowest finite (recorded, device): {[(float(want[i]), float(got[i])) for i in low]}")
    for cls in (np.isnan, np.isposinf, np.isneginf):
        np.testing.assert_array_equal(cls(got[rest]), cls(want[rest]))
    err = np.abs(got[fin] - want[fin])
    print(f"{name}: max |device - float64| over {int(fin.sum())} finite entries: {err.max():.3e} dB")
    assert err.max() <= SNR_TOL_DB


@pytest.mark.parametrize("name", ["small", "edges"])
def test_collect_weights_matches_the_recorded_lists(dev, fx, name):
    """mus bit for bit, sigmas against the recorded float64 log(1 + exp(rho)) at rtol 2e-6; where the reference's own fp32
    sigma (GaussianNode.sigma, recorded as f32_sigma_inf) is +inf -- rho = 89 -- the device's is +inf as well."""
    net, sd, _ = _device_net(fx, name, dev)
    mus, sigmas = posthoc.collect_weights(net, bnn=True)
    assert mus.cpu().numpy().tobytes() == fx[f"G11/{name}/mus"].tobytes()
    got, want = sigmas.cpu().numpy().astype(np.float64), fx[f"G11/{name}/sigmas"]
    inf32 = _bits(fx, name, "f32_sigma_inf", want.size)
    assert np.isposinf(got[inf32]).all() and (want[inf32] == 89.0).all()
    rho = C.flat_order(sd, "rho")
    print(f"{name}: sigma at rho <= -100 (recorded, device): {[(float(a), float(b)) for a, b in zip(want[rho <= -100], got[rho <= -100])]}")
    nz = ~inf32 & (want != 0)
    print(f"{name}: max rel sigma error {np.max(np.abs(got[nz] / want[nz] - 1)):.3e}")
    np.testing.assert_allclose(got[~inf32], want[~inf32], rtol=2e-6)


@pytest.mark.parametrize("name", ["small", "large", "edges", "nan"])
def test_prune_weights_with_the_recorded_list(dev, fx, name):
    """posthoc.prune_weights(net, snrs=<the reference's list>, drop): the threshold is np.percentile's bit for bit (NaN
    where the reference's is NaN: then both mask everything); the network under the band rule."""
    for di, d in enumerate(C.DROPS):
        net, sd, snr = _device_net(fx, name, dev)
        thr = posthoc.prune_weights(net, list(snr), d)
        want = float(fx[f"G11/{name}/thresholds"][di])
        assert np.float64(thr).tobytes() == np.float64(want).tobytes() or (np.isnan(thr) and np.isnan(want))
        _assert_band_rule(fx, name, di, sd, _state(net), snr, C.BAND_DB, "list")


@pytest.mark.parametrize("name", ["small", "large", "edges"])
def test_prune_weights_with_device_snrs(dev, fx, name):
    """posthoc.prune_weights(net, None, drop): the device threshold within 3e-5 dB of the recorded one, the band 2 x 3e-5.
    Where the recorded threshold is NaN (the edge network at drop 0 and 1: two -inf at the bottom and +inf at the top of the
    list, np.percentile's inf - inf; the reference then masks EVERYTHING, kept = 0 recorded) this side takes the order
    statistic: -inf keeps exactly the entries the reference's own fp32 arithmetic puts above -inf, +inf keeps none."""
    for di, d in enumerate(C.DROPS):
        net, sd, snr = _device_net(fx, name, dev)
        thr = posthoc.prune_weights(net, None, d)
        want = float(fx[f"G11/{name}/thresholds"][di])
        after = _state(net)
        print(f"device {name} drop {d}: threshold {thr!r} recorded {want!r}")
        if np.isfinite(want):
            assert abs(thr - want) <= C.BAND_DB
            _assert_band_rule(fx, name, di, sd, after, snr, 2 * C.BAND_DB, "device")
        else:
            assert name == "edges" and int(fx[f"G11/{name}/kept"][di]) == 0
            assert thr == (-np.inf if d == 0.0 else np.inf)
            above = _bits(fx, name, "f32_above_neg_inf", snr.size)
            np.testing.assert_array_equal(_keep(sd, after), above if d == 0.0 else np.zeros_like(above))


@pytest.mark.parametrize("name", ["small", "large", "edges", "lr"])
def test_snr_thresholds_match_the_recorded_percentiles(dev, fx, name):
    net, _, _ = _device_net(fx, name, dev)
    got = posthoc.snr_thresholds(net, C.DROPS).cpu().numpy()
    want = fx[f"G11/{name}/thresholds"]
    print(f"{name}: thresholds {got} recorded {want}")
    fin = np.isfinite(want)
    assert fin.sum() >= 4
    np.testing.assert_allclose(got[fin], want[fin], rtol=0, atol=C.BAND_DB)
    single = np.asarray([posthoc.snr_threshold(posthoc.compute_snr(net), d) for d in C.DROPS])
    np.testing.assert_array_equal(got, single)


def _nan_last_percentile(snr, d):
    """The order statistic this project documents: sorted with NaN last, linear interpolation."""
    v = np.sort(snr)
    pos = (v.size - 1) * d
    lo = int(np.floor(pos))
    hi = min(lo + 1, v.size - 1)
    return v[lo] if v[lo] == v[hi] else v[lo] + (v[hi] - v[lo]) * (pos - lo)


def test_a_nan_in_the_list_orders_last_here(dev, fx):
    """DELIBERATE difference.  Recorded reference result: with one NaN mu and one NaN rho np.percentile is NaN at every drop
    and prune_weights masks all 1202 elements (G11/nan: thresholds all NaN, kept all 0).  Here NaN orders last
    (bnn_snr_select, torch.sort): the thresholds are the order statistics of the list, the NaN elements are pruned (NaN >
    t is False) and every other element follows its SNR."""
    assert np.isnan(fx["G11/nan/thresholds"]).all() and not fx["G11/nan/kept"].any()
    for d in (0.25, 0.5, 0.95):
        net, sd, snr = _device_net(fx, "nan", dev)
        assert int(np.isnan(snr).sum()) == 2
        want = _nan_last_percentile(snr, d)
        assert abs(float(posthoc.snr_thresholds(net, (d,))[0]) - want) <= C.BAND_DB
        thr = posthoc.prune_weights(net, None, d)
        assert abs(thr - want) <= C.BAND_DB
        keep = _keep(sd, _state(net))
        with np.errstate(invalid="ignore"):
            ref_keep, band = snr > want, np.abs(snr - want) <= 2 * C.BAND_DB
        assert not keep[np.isnan(snr)].any() and band.sum() <= 2
        assert not ((keep != ref_keep) & ~band).any()


def test_a_local_reparam_network_is_pruned_here(dev, fx):
    """DELIBERATE difference.  Recorded reference result: prune_weights touches only BayesianLinear, a local_reparam=True
    network comes back bit for bit unchanged at every drop (G11/lr/unchanged = 1).  Here its (mu, rho) pairs are pruned like
    any other: with the reference's own list the threshold is the recorded one and the survivors are snr > threshold."""
    assert int(fx["G11/lr/unchanged"]) == 1
    for di, d in enumerate(C.DROPS[1:-1], start=1):
        net, sd, snr = _device_net(fx, "lr", dev)
        thr = posthoc.prune_weights(net, list(snr), d)
        want = float(fx["G11/lr/thresholds"][di])
        assert np.float64(thr).tobytes() == np.float64(want).tobytes()
        keep = _keep(sd, _state(net))
        out, band = C.band_differs(keep, snr > want, snr, want, C.BAND_DB)
        assert out.size == 0 and band <= 1 and 0 < keep.sum() < keep.size
        assert abs(int(keep.sum()) - round((1 - d) * snr.size)) <= 1
