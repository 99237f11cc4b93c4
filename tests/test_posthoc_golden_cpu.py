"""F3 / F4 oracle parity, no GPU: the restatements O.ece_reference, O.compute_snr and O.prune_weights against
tests/golden/posthoc.npz, which oracle/make_golden_posthoc.py recorded from the REAL compute_ece.py and weight_pruning.py
(groups G10, G11).  Plus three sensitivity checks: a restatement with one deliberate error must disagree with the fixture
on a named case -- the evidence that tests/test_gpu_posthoc.py would catch the same error in the kernel."""
import os
import warnings

import numpy as np
import pytest
import torch

import posthoc_cases as C
from oracle import bnn_oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPARED = [n for n, (_, compared, _) in C.ECE_CASES.items() if compared]
RAISING = [n for n, (_, compared, _) in C.ECE_CASES.items() if not compared]
PRUNED_NETS = ["small", "large", "edges", "nan"]


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(REPO, "tests", "golden", "posthoc.npz"))


# ------------------------------------------------------------------------------------------------------------- inputs
@pytest.mark.parametrize("name", list(C.ECE_CASES))
def test_ece_inputs_hash_to_the_fixture(fx, name):
    p, y, step, classes = C.ece_case(name)
    assert p.dtype == np.float32 and y.dtype == np.int64
    np.testing.assert_array_equal(C.sha256(p, y), fx[f"G10/{name}/sha256"])
    assert (p.shape[0], classes, step) == (int(fx[f"G10/{name}/n"]), int(fx[f"G10/{name}/classes"]), float(fx[f"G10/{name}/step"]))
    if C.ECE_CASES[name][2]:
        assert p.tobytes() == fx[f"G10/{name}/probs"].tobytes() and np.array_equal(y, fx[f"G10/{name}/labels"])


@pytest.mark.parametrize("name", list(C.SNR_NETS))
def test_network_inputs_hash_to_the_fixture(fx, name):
    dims, lr, sd = C.snr_net(name)
    np.testing.assert_array_equal(C.state_hash(sd), fx[f"G11/{name}/sha256"])
    if C.SNR_NETS[name][3]:
        assert C.flat12(sd).tobytes() == fx[f"G11/{name}/in"].tobytes()
        back = C.unflat12(fx[f"G11/{name}/in"], dims, lr)
        assert all(back[k].tobytes() == sd[k].tobytes() and back[k].shape == sd[k].shape for k in sd)


def test_the_on_edge_rows_are_what_the_case_says():
    p, y, _, _ = C.ece_case("edge_s10")
    assert list(p[C.TIE_ROWS[0]]) == [0.5, 0.5] and list(p[C.TIE_ROWS[1]]) == [0.5, 0.5] and (y[C.TIE_ROWS[0]], y[C.TIE_ROWS[1]]) == (0, 1)
    col = p[:33, 0].reshape(11, 3)
    for k in range(11):
        assert col[k, 1] == np.float32(k / 10) and col[k, 0] < col[k, 1] < col[k, 2]
        assert np.nextafter(col[k, 0], np.float32(2)) == col[k, 1] == np.nextafter(col[k, 2], np.float32(-1))
    assert col[10, 2] == np.float32(1 + 2.0 ** -23) and list(p[35]) == [0.0, 1.0] and list(p[36]) == [1.0, 0.0]


# ---------------------------------------------------------------------------------------------------------------- ECE
@pytest.mark.parametrize("name", COMPARED)
def test_ece_restatement_reproduces_the_reference(fx, name):
    p, y, step, classes = C.ece_case(name)
    assert str(fx[f"G10/{name}/raised"]) == ""
    ece, centers, acc, (cnt, _, _) = O.ece_reference(p, y, step, classes)
    assert (cnt > 0).all()
    np.testing.assert_allclose(ece, fx[f"G10/{name}/ece"], rtol=1e-12)
    np.testing.assert_allclose(centers, fx[f"G10/{name}/centers"], rtol=1e-12)
    np.testing.assert_allclose(acc, fx[f"G10/{name}/bin_acc"], rtol=1e-12)


@pytest.mark.parametrize("name", RAISING)
def test_ece_restatement_is_nan_where_the_reference_raises(fx, name):
    """Recorded: IndexError for n = 1, for the sparse 257 x 37 case and for ANY input at bin_step 0.05 (np.arange(0, 1.1,
    0.05) has 22 edges; the bin (1.0, 1.05] is always empty).  The restatement catches exactly that error as NaN."""
    p, y, step, classes = C.ece_case(name)
    assert str(fx[f"G10/{name}/raised"]) == "IndexError"
    ece, centers, acc, (cnt, _, _) = O.ece_reference(p, y, step, classes)
    assert np.isnan(ece) and not (cnt > 0).all() and len(centers) == len(acc) == int((cnt > 0).sum())


def test_extreme_cases_have_the_accuracies_they_are_named_for(fx):
    assert not fx["G10/all_wrong/bin_acc"].any()
    acc = fx["G10/all_right/bin_acc"]                       # a correct row counts its argmax only: the top bins reach 1
    assert acc.max() == 1.0 and (acc >= 0).all()


# ------------------------------------------------------------------------------------------------------ sensitivity
def _ece_variant(p, y, step, classes, edges32=False, last_max=False, drop_tail=False):
    """A plain restatement of ECELoss.forward with one deliberate error switched on at a time: the bin edges rounded to
    fp32, the LAST maximum as the predicted class, the rows after the last full 64 dropped."""
    if drop_tail:
        p, y = p[:p.shape[0] // 64 * 64], y[:p.shape[0] // 64 * 64]
    n = p.shape[0]
    pred = (classes - 1 - np.argmax(p[:, ::-1], axis=1)) if last_max else np.argmax(p, axis=1)
    edges = np.arange(0, 1.1, step)
    flat = p.reshape(-1).astype(np.float64)
    if edges32:
        edges = edges.astype(np.float32).astype(np.float64)
    idx = np.digitize(flat, edges, right=True) - 1
    correct = np.zeros((n, classes), np.int64)
    correct[np.arange(n), pred] = pred == y
    correct = correct.reshape(-1)
    nb = len(edges) - 1
    cnt = np.asarray([(idx == b).sum() for b in range(nb)], np.float64)
    cor = np.asarray([correct[idx == b].sum() for b in range(nb)], np.float64)
    conf = np.asarray([flat[idx == b].sum() for b in range(nb)], np.float64)
    have = cnt > 0
    ece = float((np.abs(conf[have] / cnt[have] - cor[have] / cnt[have]) * cnt[have] / cnt.sum()).sum())
    return ece, cor[have] / cnt[have]


def _agrees(fx, name, **err):
    p, y, step, classes = C.ece_case(name)
    ece, acc = _ece_variant(p, y, step, classes, **err)
    want_acc = fx[f"G10/{name}/bin_acc"]
    return bool(np.isclose(ece, fx[f"G10/{name}/ece"], rtol=1e-6, atol=0)) and acc.shape == want_acc.shape and bool((acc == want_acc).all())


@pytest.mark.parametrize("name", COMPARED)
def test_the_unbroken_variant_agrees_everywhere(fx, name):
    assert _agrees(fx, name)


@pytest.mark.parametrize("err,name", [("edges32", "edge_s10"), ("last_max", "edge_s10"), ("drop_tail", "n65")])
def test_one_deliberate_error_is_caught_by_its_named_case(fx, err, name):
    """fp32 edges move float32(0.1) (> 0.1 in float64, == the fp32 edge) into the bin below; the last maximum turns the
    (0.5, 0.5) rows' predicted class from 0 to 1; dropping the rows after the last full 64 loses row 64 of n = 65."""
    assert not _agrees(fx, name, **{err: True})


# ------------------------------------------------------------------------------------------------------- SNR, pruning
def _recorded_state(fx, name):
    dims, lr, sd = C.snr_net(name)                          # (hash-checked above; the small ones are also stored whole)
    return dims, lr, sd


@pytest.mark.parametrize("name", ["small", "edges", "nan", "lr"])
def test_snr_restatement_reproduces_the_float64_list(fx, name):
    _, _, sd = _recorded_state(fx, name)
    mus = C.flat_order(sd, "mu")
    assert mus.tobytes() == fx[f"G11/{name}/mus"].tobytes()                     # collect_weights' order, bit for bit
    with np.errstate(all="ignore"):
        sig = np.log(1 + np.exp(C.flat_order(sd, "rho").astype(np.float64)))    # rho_to_sigma, weight_pruning.py:40-41
        snr = O.compute_snr(mus.astype(np.float64), sig)
    if f"G11/{name}/sigmas" in fx:
        np.testing.assert_allclose(sig, fx[f"G11/{name}/sigmas"], rtol=1e-12)
    want = fx[f"G11/{name}/snr"]
    fin = np.isfinite(want)
    np.testing.assert_allclose(snr[fin], want[fin], rtol=1e-12)
    np.testing.assert_array_equal(snr[~fin], want[~fin])                         # the same +-inf / NaN at the same places


def _snr64(fx, name, sd):
    if f"G11/{name}/snr" in fx:
        return fx[f"G11/{name}/snr"]
    with np.errstate(all="ignore"):
        snr = O.compute_snr(C.flat_order(sd, "mu").astype(np.float64), np.log(1 + np.exp(C.flat_order(sd, "rho").astype(np.float64))))
    return snr


def test_large_snr_list_hashes_to_the_fixture(fx):
    """The 119-100-10 network's float64 list is recorded as its sha256 only: the restated list has those bytes, and its
    percentiles are the recorded thresholds."""
    _, _, sd = _recorded_state(fx, "large")
    snr = _snr64(fx, "large", sd)
    np.testing.assert_array_equal(C.sha256(snr), fx["G11/large/snr_sha256"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        thr = np.asarray([np.percentile(snr, 100 * d) for d in C.DROPS])
    np.testing.assert_allclose(thr, fx["G11/large/thresholds"], rtol=1e-12)


def _canon(a):
    """fp32 bits with every NaN as one pattern: inf * 0 is the NaN of the machine that multiplies (sign and payload are
    not IEEE's to fix), everything else -- signed zeros included -- is compared bit for bit."""
    bits = np.ascontiguousarray(a, np.float32).view(np.int32).copy()
    bits[np.isnan(a)] = 0x7FC00000
    return bits


@pytest.mark.parametrize("name", PRUNED_NETS)
def test_prune_restatement_reproduces_the_reference(fx, name):
    dims, lr, sd = _recorded_state(fx, name)
    snr = _snr64(fx, name, sd)
    layers = [tuple(torch.from_numpy(sd[f"{l}.{n}"]) for n in C.PARAMS) for l in C.LAYERS]
    rho = C.flat_order(sd, "rho")
    for di, d in enumerate(C.DROPS):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            got, thr = O.prune_weights(layers, snr, d)
        want_thr = float(fx[f"G11/{name}/thresholds"][di])
        assert (np.isnan(thr) and np.isnan(want_thr)) or np.isclose(thr, want_thr, rtol=1e-12, atol=0)
        after = {f"{l}.{n}": t.numpy() for l, ts in zip(C.LAYERS, got) for n, t in zip(C.PARAMS, ts)}
        ra = C.flat_order(after, "rho")
        keep = (ra != 0) & ~np.isnan(rho) & ~np.isnan(C.flat_order(after, "mu"))
        ref_keep = np.unpackbits(fx[f"G11/{name}/keep/{di}"])[:keep.size].astype(bool)
        out_of_band, band = C.band_differs(keep, ref_keep, snr, want_thr, C.BAND_DB)
        assert out_of_band.size == 0 and band == int(fx[f"G11/{name}/band"][di]) <= max(1, keep.size // 1000)
        assert int(fx[f"G11/{name}/kept"][di]) == int(ref_keep.sum())
        key = f"G11/{name}/pruned/{0 if name == 'nan' else di}"
        if key in fx:                                       # the small networks: all twelve tensors, bit for bit in the band's complement
            diff = np.flatnonzero(_canon(C.flat12(after)) != _canon(fx[key]))
            assert diff.size <= 4 * band, (name, d, diff)


def test_recorded_reference_behaviour_no_test_stated_before(fx):
    """What the recording shows beyond the values: a NaN anywhere in the list makes every threshold NaN and the reference
    masks every element; a local_reparam network comes back unchanged (prune_weights only touches BayesianLinear); two
    -inf at the bottom or a +inf at the top of the list make np.percentile NaN at drop 0 / 1; at rho = 89 the reference's
    two arithmetics part: the float64 list holds 10 log10(|mu| / 89), its fp32 torch mask sees sigma = +inf, SNR = -inf."""
    assert np.isnan(fx["G11/nan/thresholds"]).all() and not fx["G11/nan/kept"].any()
    assert int(fx["G11/lr/unchanged"]) == 1 and np.isfinite(fx["G11/lr/thresholds"]).all()
    thr = fx["G11/edges/thresholds"]
    assert np.isnan(thr[0]) and np.isnan(thr[-1]) and np.isfinite(thr[1:-1]).all()
    _, _, sd = C.snr_net("edges")
    rho, snr = C.flat_order(sd, "rho"), fx["G11/edges/snr"]
    above = np.unpackbits(fx["G11/edges/f32_above_neg_inf"])[:rho.size].astype(bool)
    sig_inf = np.unpackbits(fx["G11/edges/f32_sigma_inf"])[:rho.size].astype(bool)
    assert (rho == 89).sum() == 3 and np.array_equal(sig_inf, rho == 89)
    assert np.isfinite(snr[rho == 89]).all() and not above[rho == 89].any()
    assert np.array_equal(np.isfinite(snr) & ~above, rho == 89)
    for n in ("small", "large"):                            # drops 0 and 1: exactly the threshold element in the band
        assert list(fx[f"G11/{n}/band"]) == [1, 0, 0, 0, 0, 1]


def test_labels_say_pinned():
    src = open(os.path.join(REPO, "oracle", "bnn_oracle.py")).read()
    assert "pinned by tests/golden/posthoc.npz" in src and "UNPINNED" not in src
    for rel in ("DESIGN.md", "INTEGRATION.md", os.path.join("tests", "test_gpu_posthoc.py"),
                os.path.join("bayesian-neural-network_amd", "bnn_hip", "posthoc.py")):
        assert "unpinned" not in open(os.path.join(REPO, rel)).read().lower().replace("-", " "), rel
