"""The fp64 loss-tail reference (tests/loss_tail_ref.py) without a device: checked against torch's own float64
cross-entropy / Normal.log_prob and autograd, and against oracle.nll; and its fp32 error bound shown to have teeth --
numpy restatements of plausible kernel mistakes must each fall outside it on the very logits the GPU tests use."""
import math

import numpy as np
import pytest
import torch

import loss_tail_ref as R
from oracle import bnn_oracle as O

# (mode, S, B, C, seed): the shapes of tests/test_gpu_loss_tail.py's sweep, cut down to what runs quickly on the CPU
CASES = [("classification", 3, 17, 1, 1), ("classification", 5, 17, 2, 2), ("classification", 5, 128, 10, 3),
         ("classification", 5, 17, 16, 4), ("classification", 5, 300, 17, 5), ("classification", 5, 17, 33, 6),
         ("classification", 5, 128, 100, 7), ("classification", 5, 17, 1000, 8),
         ("regression", 3, 17, 1, 9), ("regression", 3, 128, 9, 10), ("regression", 3, 17, 65, 11), ("regression", 2, 17, 4096, 12)]
SIGMA = 0.7


def _inputs(mode, S, B, C, seed, groups=1):
    lg = R.make_logits(S, B, C, seed, special=mode == "classification")
    tg = R.make_labels(B, C, seed, groups) if mode == "classification" else R.make_reg_targets(B, C, seed, groups)
    return lg, tg


@pytest.mark.parametrize("mode,S,B,C,seed", CASES)
def test_reference_matches_torch_float64(mode, S, B, C, seed):
    lg, tg = _inputs(mode, S, B, C, seed)
    x = torch.from_numpy(lg).double().requires_grad_(True)
    if mode == "classification":
        t = torch.from_numpy(tg[0])
        per = torch.stack([torch.nn.functional.cross_entropy(x[s], t, reduction="sum") for s in range(S)])
    else:
        t = torch.from_numpy(tg[0]).double()
        per = torch.stack([-torch.distributions.Normal(x[s], SIGMA).log_prob(t).sum() for s in range(S)])
    gs = np.linspace(0.25, 1.5, S)
    (per * torch.from_numpy(gs)).sum().backward()
    want = per.detach().numpy()
    got = R.nll(lg, tg, mode, SIGMA)
    assert np.allclose(got, want, rtol=1e-12, atol=1e-9)
    assert np.allclose(R.nll_grad(lg, tg, mode, SIGMA, gs), x.grad.numpy(), rtol=1e-10, atol=1e-13)
    # the fp32 restatement of networks.py:183-190 (oracle.nll, torch's fp32 kernels) lies within the bound
    for s in range(S):
        o = float(O.nll(torch.from_numpy(lg[s]), torch.from_numpy(tg[0]), mode, SIGMA))
        if mode == "classification" and np.abs(lg[s]).max() > 500:
            continue    # (torch's fp32 CE on the 1e3-offset rows: its own rounding of |m| ~ 1e3, not a property of the bound)
        assert abs(o - got[s]) <= R.nll_tol(lg[s:s + 1], tg, mode, SIGMA)[0], (s, o, got[s])


def test_special_rows_have_their_closed_forms():
    C = 33
    lg = R.make_logits(5, 4, C, 0)
    tg = np.zeros((1, 4), np.int64)
    rows = R.nll_rows(lg, tg, "classification")
    for s in range(5):
        for b in range(4):
            kind = R.SPECIAL_KINDS[(s + b) % 5]
            if kind == "equal":
                assert rows[s, b] == pytest.approx(math.log(C), rel=1e-15)
            if kind == "offset":
                assert np.isfinite(rows[s, b]) and lg[s, b].min() > 900
    assert np.isfinite(rows).all()


def test_per_group_targets_pick_their_own_group():
    S, g, B, C = 6, 2, 5, 7
    lg = R.make_logits(S, B, C, 3)
    tg = R.make_labels(B, C, 3, groups=S // g)
    got = R.nll(lg, tg, "classification")
    for s in range(S):
        assert got[s] == R.nll(lg[s:s + 1], tg[s // g][None], "classification")[0]
    assert (R.per_sample_targets(tg, S)[::g] == tg).all()


def test_bad_labels_poison_only_their_rows():
    lg = R.make_logits(2, 6, 10, 1)
    tg = R.make_labels(6, 10, 1)
    tg[0, 2], tg[0, 4] = -1, 10
    rows = R.nll_rows(lg, tg, "classification")
    assert np.isnan(rows[:, [2, 4]]).all() and np.isfinite(rows[:, [0, 1, 3, 5]]).all()
    g = R.nll_grad(lg, tg, "classification")
    assert np.isnan(g[:, [2, 4]]).all() and np.isfinite(g[:, [0, 1, 3, 5]]).all()


def test_loss_assembly_matches_the_reference_elbo():
    rs = np.random.RandomState(0)
    S = 7
    a, b, n = rs.standard_normal(S) * 1e4, rs.standard_normal(S) * 1e4, rs.uniform(10, 200, S)
    for beta in (0.0, 2.0 ** -10, 0.5):
        out4, g_a, g_b, g_kl3 = R.loss_assembly(a, b, n, beta, S, 0.5, False)
        assert out4[0] == pytest.approx(beta * b.mean() - beta * a.mean() + n.mean(), rel=1e-14, abs=1e-12)   # networks.py:205-208
        assert (g_a == -beta * 0.5 / S).all() and (g_b == beta * 0.5 / S).all() and g_kl3[0] == beta * 0.5
        out4, g_a, _, _ = R.loss_assembly(a, None, n, beta, 2 * S, 1.0, True)
        assert out4[0] == pytest.approx(beta * a.sum() / (2 * S) + n.sum() / (2 * S), rel=1e-14, abs=1e-12)    # :222-224
        assert (g_a == 0).all() and out4[2] == 0
    sums = R.elbo_sums(a[:6], b[:6], n[:6], 3)
    assert sums.shape == (2, 4) and sums[1, 2] == pytest.approx(n[3:6].sum()) and (sums[:, 3] == 3).all()


# ------------------------------------------------------------------------------------------------ mutations: the bound has teeth
def _fp32_nll(lg, tg, mode, sigma=SIGMA, label_shift=0, drop_last=False, no_max=False, group_stride0=False,
              no_log_sigma=False):
    """An fp32 numpy restatement of fin_nll's arithmetic with one optional mistake switched on."""
    S, B, C = lg.shape
    t = R.per_sample_targets(tg[:1] if group_stride0 else tg, S)
    out = np.zeros(S, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(S):
            x = lg[s].astype(np.float32)
            if mode == "classification":
                xs = x[:, :C - 1] if (drop_last and C > 1) else x
                m = np.zeros(B, np.float32) if no_max else xs.max(1)
                se = np.exp(xs - m[:, None]).sum(1, dtype=np.float32)
                lab = np.clip(t[s] + label_shift, 0, C - 1) if label_shift else t[s]
                pk = x[np.arange(B), lab]
                rows = (m + np.log(se)) - pk
            else:
                d = t[s].astype(np.float32) - x
                c = (0.0 if no_log_sigma else math.log(sigma)) + R.C0
                rows = (d * d / np.float32(2 * sigma * sigma) + np.float32(c)).sum(1, dtype=np.float32)
            out[s] = rows.astype(np.float64).sum()
    return out


def _outside(got, want, tol):
    return bool((~np.isfinite(got)).any() or (np.abs(got - want) > tol).any())


@pytest.mark.parametrize("mode,S,B,C,seed", CASES)
def test_fp32_restatement_meets_the_bound(mode, S, B, C, seed):
    """The guard of every mutation below: with the mistake switched off the fp32 arithmetic is inside the bound."""
    lg, tg = _inputs(mode, S, B, C, seed)
    assert not _outside(_fp32_nll(lg, tg, mode), R.nll(lg, tg, mode, SIGMA), R.nll_tol(lg, tg, mode, SIGMA))


@pytest.mark.parametrize("mutation", ["label_off_by_one", "lse_over_c_minus_1", "no_max_subtraction", "group_stride_0"])
@pytest.mark.parametrize("mode,S,B,C,seed", [c for c in CASES if c[0] == "classification" and c[3] > 1])
def test_classification_mutations_fall_outside_the_bound(mode, S, B, C, seed, mutation):
    groups = 5 if mutation == "group_stride_0" else 1
    lg, tg = _inputs(mode, S, B, C, seed, groups)
    want, tol = R.nll(lg, tg, mode), R.nll_tol(lg, tg, mode)
    kw = {"label_off_by_one": dict(label_shift=1), "lse_over_c_minus_1": dict(drop_last=True),
          "no_max_subtraction": dict(no_max=True), "group_stride_0": dict(group_stride0=True)}[mutation]
    assert not _outside(_fp32_nll(lg, tg, mode), want, tol)          # the guard
    assert _outside(_fp32_nll(lg, tg, mode, **kw), want, tol), mutation


@pytest.mark.parametrize("mutation", ["no_log_sigma", "group_stride_0"])
@pytest.mark.parametrize("mode,S,B,C,seed", [c for c in CASES if c[0] == "regression"])
def test_regression_mutations_fall_outside_the_bound(mode, S, B, C, seed, mutation):
    groups = S if mutation == "group_stride_0" else 1
    lg, tg = _inputs(mode, S, B, C, seed, groups)
    want, tol = R.nll(lg, tg, mode, SIGMA), R.nll_tol(lg, tg, mode, SIGMA)
    assert not _outside(_fp32_nll(lg, tg, mode), want, tol)
    assert _outside(_fp32_nll(lg, tg, mode, **{mutation.replace("group_stride_0", "group_stride0"): True}), want, tol), mutation


def test_gradient_bound_has_teeth():
    """The elementwise gradient bound: the fp32 restatement inside it, a label off by one and a softmax over C-1
    classes outside it."""
    for C in (2, 10, 33, 1000):
        lg = R.make_logits(3, 17, C, C)
        tg = R.make_labels(17, C, C)
        want, tol = R.nll_grad(lg, tg, "classification", gs=0.5), R.nll_grad_tol(lg, tg, "classification", gs=0.5)
        x = lg.astype(np.float32)
        m = x.max(-1, keepdims=True)
        e = np.exp(x - m)
        oh = (np.arange(C)[None, None] == tg[0][None, :, None]).astype(np.float32)
        got = (e * (np.float32(1) / e.sum(-1, keepdims=True, dtype=np.float32)) - oh) * np.float32(0.5)
        assert (np.abs(got - want) <= tol).all()
        oh1 = (np.arange(C)[None, None] == ((tg[0] + 1) % C)[None, :, None]).astype(np.float32)
        assert (np.abs((e / e.sum(-1, keepdims=True) - oh1) * 0.5 - want) > tol).any()
        e1 = e.copy()
        e1[..., -1] = 0
        assert (np.abs((e1 / e1.sum(-1, keepdims=True) - oh) * 0.5 - want) > tol).any()
