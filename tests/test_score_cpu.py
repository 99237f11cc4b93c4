"""CPU-side checks of the held-out scores (bnn_mc_score, F12; no GPU): the ctypes mirror and the record macros match the
header, the host rejects bad arguments before any launch, the float64 restatement the GPU tests compare against agrees with
torch's own losses, and Scores.read() / coverage() parse hand-written records."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import score_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "bnn_hip.h")


def test_score_struct_layout_matches_the_header(tmp_path):
    from bnn_hip import _lib
    cls, cname = _lib.McScoreArgs, "bnn_mc_score_args"
    lines = ['printf("%%zu\\n", sizeof(%s));' % cname]
    want = [C.sizeof(cls)]
    for fname, _t in cls._fields_:
        lines.append('printf("%%zu\\n", offsetof(%s, %s));' % (cname, fname))
        want.append(getattr(cls, fname).offset)
    lines.append('printf("%d\\n", BNN_SCORE_MAX_BINS);')
    lines.append('printf("%d\\n", (int)BNN_SCORE_RECORD_BYTES(10));')
    want += [_lib.SCORE_MAX_BINS, _lib.score_record_bytes(10)]
    assert _lib.score_record_bytes(10) == 8 * 38
    prog = tmp_path / "sz.c"
    prog.write_text('#include "%s"\n#include <stdio.h>\n#include <stddef.h>\nint main(){%s return 0;}' % (HEADER, "".join(lines)))
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", str(prog), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == want


def test_abi_version_is_still_9_and_the_names_are_declared():
    from bnn_hip import _lib as L
    lib = L.load()
    assert lib.bnn_version() == 9 and L.ABI_VERSION == 9
    assert "bnn_mc_score" in L.EXPORTS and "bnn_mc_score_workspace_bytes" in L.EXPORTS


def _valid_args(L, mode):
    fake = 0x1000
    a = L.McScoreArgs()
    a.struct_bytes, a.mode = C.sizeof(L.McScoreArgs), mode
    a.groups, a.n_samples, a.batch, a.classes = 2, 4, 8, 3
    a.logits, a.targets, a.record, a.workspace = fake, fake, fake, fake
    a.n_valid, a.sigma, a.n_bins = 16, 0.5, 10
    a.workspace_bytes = L.load().bnn_mc_score_workspace_bytes(2, 8, 3)
    return a


def test_score_argument_validation_without_a_device():
    """Every check runs on the host before a launch (fake, never dereferenced device addresses).  Each case starts from
    arguments that pass every check and breaks one thing; the last assertion of a case restores it."""
    from bnn_hip import _lib as L
    lib = L.load()
    call = lambda a: lib.bnn_mc_score(C.byref(a), None)            # noqa: E731
    assert lib.bnn_mc_score_workspace_bytes(2, 8, 3) > 0
    assert lib.bnn_mc_score_workspace_bytes(0, 8, 3) == 0 and lib.bnn_mc_score_workspace_bytes(2, -1, 3) == 0
    assert lib.bnn_mc_score_workspace_bytes(2, 8, 100) > lib.bnn_mc_score_workspace_bytes(2, 8, 3)

    a = L.McScoreArgs()
    assert call(a) == -5                                            # struct_bytes mismatch
    a = _valid_args(L, L.NLL_CLASSIFICATION)
    a.struct_bytes -= 8
    assert call(a) == -5
    for mode in (L.NLL_CLASSIFICATION, L.NLL_REGRESSION):
        a = _valid_args(L, mode)
        a.mode = 7
        assert call(a) == -3                                        # unknown mode
        for dim in ("groups", "n_samples", "batch", "classes"):
            for bad in (0, -1):
                a = _valid_args(L, mode)
                setattr(a, dim, bad)
                assert call(a) == -2, (dim, bad)                    # zero or negative shape
        for bad in (0, -3, 17):
            a = _valid_args(L, mode)
            a.n_valid = bad
            assert call(a) == -2, bad                               # n_valid outside 1 .. G * B
        for bad in (-1, L.SCORE_MAX_BINS + 1):
            a = _valid_args(L, mode)
            a.n_bins = bad
            assert call(a) == -2, bad                               # n_bins outside 0 .. BNN_SCORE_MAX_BINS
        for ptr in ("logits", "targets", "record"):
            a = _valid_args(L, mode)
            setattr(a, ptr, None)
            assert call(a) == -1, ptr                               # NULL logits / targets / record
        a = _valid_args(L, mode)
        a.workspace_bytes -= 1
        assert call(a) == -1                                        # workspace too small
        a.workspace_bytes += 1
        a.workspace = None
        assert call(a) == -1
        a = _valid_args(L, mode)
        a.record = 0x1004
        assert call(a) == -6                                        # misaligned record
    a = _valid_args(L, L.NLL_CLASSIFICATION)
    a.targets = 0x1004
    assert call(a) == -6                                            # misaligned int64 targets
    a.sigma = 0.0                                                   # sigma is a regression argument: the order of the checks
    assert call(a) == -6
    for bad in (0.0, -1.0, float("nan")):
        a = _valid_args(L, L.NLL_REGRESSION)
        a.sigma = bad
        assert call(a) == -2, bad                                   # regression sigma must be > 0
    a = _valid_args(L, L.NLL_REGRESSION)
    a.sigma, a.logits = 0.0, None
    assert call(a) == -2                                            # the shape checks come before the pointer checks


def _class_case(seed, G=2, S=5, B=9, C=7):
    rng = np.random.default_rng(seed)
    lg = (rng.standard_normal((G, S, B, C)) * 3).astype(np.float32)
    y = rng.integers(0, C, size=(G, B))
    return lg, y


def _reg_case(seed, G=2, S=5, B=9, C=3):
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((G, S, B, C)).astype(np.float32)
    y = rng.standard_normal((G, B, C)).astype(np.float32)
    return f, y


def test_restatement_nll_is_torchs_cross_entropy_and_normal_log_prob():
    """sum nll = the mean over s of the reference's get_nll(output_s, target): CrossEntropyLoss(reduction='sum') and
    -Normal(out, sigma).log_prob(y).sum(), both in fp64."""
    lg, y = _class_case(1)
    G, S, B, Cc = lg.shape
    ref = score_ref.classification(lg, y, 10)
    ce = torch.nn.CrossEntropyLoss(reduction="sum")
    want = sum(float(ce(torch.from_numpy(lg[g, s]).double(), torch.from_numpy(y[g]))) for g in range(G) for s in range(S)) / S
    np.testing.assert_allclose(ref["sum_nll"], want, rtol=1e-12)
    f, t = _reg_case(2)
    for sigma in (0.1, 1.0):
        sg = float(np.float32(sigma))
        ref = score_ref.regression(f, t, sigma, 10)
        want = sum(float(-torch.distributions.Normal(torch.from_numpy(f[g, s]).double(), sg).log_prob(torch.from_numpy(t[g]).double()).sum())
                   for g in range(f.shape[0]) for s in range(f.shape[1])) / f.shape[1]
        np.testing.assert_allclose(ref["sum_nll"], want, rtol=1e-12)


def test_jensen_lpd_is_at_least_minus_nll_with_equality_at_one_sample():
    for S in (1, 5):
        lg, y = _class_case(3, S=S)
        c = score_ref.classification(lg, y, 10)
        f, t = _reg_case(4, S=S)
        r = score_ref.regression(f, t, 0.1, 10)
        for ref in (c, r):
            assert (ref["lpd"] >= -ref["nll"] - 1e-12 * np.maximum(1.0, np.abs(ref["nll"]))).all()
            if S == 1:
                np.testing.assert_allclose(ref["lpd"], -ref["nll"], rtol=1e-13, atol=1e-13)
            else:
                assert (ref["lpd"] > -ref["nll"]).any()


def test_restatement_edge_cases():
    """A softmax that underflows in fp32 keeps a finite lpd; a label outside [0, C) gives -inf; a NaN row goes to no bin; a
    target 50 sigma from every sample has a finite lpd and a PIT in an outer bin; padding is excluded by n_valid."""
    lg, y = _class_case(5, G=1, S=3, B=4, C=3)
    lg[0, :, 0] = [[80.0, 80.5, -80.0]] * 3
    y[0, 0] = 2
    y[0, 1] = 3                                                     # out of range
    lg[0, 1, 2, 0] = np.nan
    ref = score_ref.classification(lg, y, 10)
    fp32 = torch.softmax(torch.from_numpy(lg[0, :, 0]), -1)[:, 2]
    assert float(fp32.max()) == 0.0 and np.isfinite(ref["lpd"][0]) and ref["lpd"][0] < -150
    assert ref["lpd"][1] == -np.inf and ref["nll"][1] == np.inf
    assert np.isnan(ref["lpd"][2]) and ref["bin"][2] == -1 and not ref["correct"][2]
    assert ref["rows"] == 4 and ref["bin_count"].sum() == 3
    short = score_ref.classification(lg, y, 10, n_valid=1)
    assert short["rows"] == 1 and np.isfinite(short["sum_lpd"]) and short["bin_count"].sum() == 1

    f, t = _reg_case(6, G=1, S=4, B=5, C=1)
    t[0, 0, 0], t[0, 1, 0] = f[0, :, 0, 0].max() + 50 * 0.1, f[0, :, 1, 0].min() - 50 * 0.1
    ref = score_ref.regression(f, t, 0.1, 10)
    assert np.isfinite(ref["lpd"][:2]).all() and ref["bin"][0] == 9 and ref["bin"][1] == 0
    assert ref["pit"][0] == 1.0 and ref["pit"][1] == 0.0
    assert score_ref._interior_margin(ref["pit"][:2], 10) == 1.0    # u = 0 and u = 1 sit on outer edges: no bin boundary


def _class_record(n_bins=4):
    w = np.zeros(8 + 3 * n_bins, np.int64)
    f = w.view(np.float64)
    w[0], w[1] = 10, 7
    f[2], f[3], f[4] = -5.0, 6.0, 2.5
    for i, (cnt, ok, conf) in enumerate([(0, 0, 0.0), (2, 1, 0.8), (3, 2, 2.1), (5, 4, 4.5)]):
        w[8 + 3 * i], w[8 + 3 * i + 1], f[8 + 3 * i + 2] = cnt, ok, conf
    return w


def test_scores_read_parses_a_handwritten_classification_record():
    from bnn_hip import ops
    r = ops.Scores("classification", bins=4, record=torch.from_numpy(_class_record())).read()
    assert r.n == 10 and r.accuracy == 0.7 and r.lpd == -0.5 and r.nll == 0.6 and r.brier == 0.25
    np.testing.assert_allclose(r.ece, (0.2 + 0.1 + 0.5) / 10, rtol=1e-15)
    np.testing.assert_allclose(r.mce, 0.1, rtol=1e-12)              # |0.8 - 1| / 2 = 0.1, |2.1 - 2| / 3, |4.5 - 4| / 5 = 0.1
    assert r.bin_count.tolist() == [0, 2, 3, 5]
    assert np.isnan(r.bin_accuracy[0]) and np.isnan(r.bin_confidence[0])
    np.testing.assert_allclose(r.bin_accuracy[1:], [0.5, 2 / 3, 0.8])
    np.testing.assert_allclose(r.bin_confidence[1:], [0.4, 0.7, 0.9])
    assert isinstance(r.lpd, float) and isinstance(r.n, int) and isinstance(r.bin_count, np.ndarray)
    with pytest.raises(ops.BnnHipError):
        ops.Scores("classification", bins=5, record=torch.from_numpy(_class_record()))
    with pytest.raises(ops.BnnHipError):
        ops.Scores("classification", bins=65, record=torch.zeros(8 + 3 * 65, dtype=torch.int64))


def test_scores_read_and_coverage_on_a_handwritten_regression_record():
    from bnn_hip import ops
    pit = [1, 2, 3, 4, 10, 20, 30, 15, 10, 5]
    w = np.zeros(8 + 30, np.int64)
    f = w.view(np.float64)
    w[0], w[1] = 50, 100
    f[2], f[3], f[4], f[5] = -120.0, 150.0, 400.0, 90.0
    w[8::3] = pit
    r = ops.Scores("regression", bins=10, record=torch.from_numpy(w)).read()
    assert r.n == 100 and r.rows == 50 and r.rmse == 2.0 and r.mae == 0.9 and r.lpd == -1.2 and r.nll == 1.5
    assert r.pit.tolist() == pit
    assert r.coverage(0.2) == 0.30 and r.coverage(0.6) == 0.82 and r.coverage(1.0) == 1.0
    np.testing.assert_allclose(r.coverage(0.8), 0.94)
    for bad in (0.5, 0.9, 0.95, 0.0, 1.2):                          # level * M / 2 is no integer in [1, M / 2]
        with pytest.raises(ops.BnnHipError):
            r.coverage(bad)
    odd = np.zeros(8 + 27, np.int64)
    odd[1] = 9
    with pytest.raises(ops.BnnHipError):
        ops.Scores("regression", bins=9, record=torch.from_numpy(odd)).read().coverage(0.5)
