"""The Kronecker-factored Laplace posterior on the device (bnn_kfac_layer / _evidence / _glm_rotate / _glm_var / _sample,
bnn_hip.kfac.KronLaplace; include/bnn_hip.h F20): every stage against its fp64 restatement (tests/kfac_ref.py) computed from the
kernel's own inputs, the accumulated factors end to end against the autograd-Jacobian reference, the accumulation semantics bit
for bit, the evidence and the chosen precision, the GLM moments against the dense fp64 J P^-1 J^T, the predictive interface, the
weight draws against the restated Philox stream, and the failure modes.

Shapes are test_gpu_laplace.py's: every edge of a 64-tile and of a 32-wide k stage is crossed, also at in + 1 = 71, 66, 101, 2,
41 -- classification 70-65-3 with batch 33 then 1, regression 1-40-1 with batch 5, classification 119-100-10 with batch 64."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bnn_hip
import kfac_ref as K
import laplace_ref as R
from bnn_hip import _lib as L
from bnn_hip import ops
from bnn_hip.ops import BnnHipError
from test_gpu_laplace import CASES, IDS, SIGMA, _batch, _bf16, _close, _mlp, _np, _relu_margin, _same, _two_batches, _weights

TAUS = (1e-2, 1.0, 1e2)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore():
    yield
    bnn_hip.set_math("bf16")
    bnn_hip.manual_seed(2026)


def _bits(la):
    return [t.clone() for t in la._accumulated()]


# ------------------------------------------------------------------------------------------------------------ 1. stage by stage
@pytest.mark.parametrize("math_mode,tol_gx", [("f32", 1e-5), ("bf16", 2e-3)])
@pytest.mark.parametrize("curvature", ["ggn", "empirical"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_stage_against_its_fp64_restatement(dev, case, curvature, math_mode, tol_gx):
    mode, inp, hid, C, batches = case
    bnn_hip.set_math(math_mode)
    mm = L.MATH_BF16 if math_mode == "bf16" else L.MATH_F32
    mlp = _mlp(dev, mode, inp, hid, C)
    lins = [m for m in mlp.net if hasattr(m, "weight")]
    fa = [torch.zeros((m.in_features, m.in_features), device=dev) for m in lins]
    fs = [torch.zeros(m.in_features, device=dev) for m in lins]
    fg = [torch.zeros((m.out_features, m.out_features), device=dev) for m in lins]
    record = torch.zeros(2, dtype=torch.float64, device=dev)
    for bi, B in enumerate(batches):
        x, y = _batch(dev, mlp, B, seed=10 + bi)
        xf = x.reshape(B, -1).contiguous()
        acts, h = [], xf
        for i, m in enumerate(lins):
            h = ops.dense_fwd(h, m.weight.detach(), m.bias.detach(), n_samples=1, math_mode=L.MATH_F32, relu=i < 2, drop_p=0.0,
                              layer_id=i, seed=0, y_dtype=torch.float32)[0]
            acts.append(h)
        g = ops.laplace_seed(acts[-1], y, mode, curvature=curvature, sigma=SIGMA, record=record)
        for i in (2, 1, 0):
            xin = xf if i == 0 else acts[i - 1]
            w = lins[i].weight.detach()
            before = [_np(fa[i]), _np(fs[i]), _np(fg[i])]
            gx = torch.full((g.shape[0], w.shape[1]), float("nan"), device=dev) if i > 0 else None
            ysv = acts[i] if i < 2 else None
            ops.kfac_layer(xin, g, w, a=fa[i], s=fs[i], g=fg[i], g_x=gx, y=ysv, gx_mask=i > 0, math_mode=mm)
            dA, ds, dG, _ = K.layer(_np(xin), _np(g), None if ysv is None else _np(ysv), _np(w), want_gx=False)
            _close(_np(fa[i]), before[0] + dA, 1e-5, f"A{i} b{B}")
            _close(_np(fs[i]), before[1] + ds, 1e-5, f"s{i} b{B}")
            _close(_np(fg[i]), before[2] + dG, 1e-5, f"G{i} b{B}")
            assert torch.equal(fa[i], fa[i].T) and torch.equal(fg[i], fg[i].T)           # bit-symmetric
            if i > 0:
                gz = _np(g).reshape(-1, B, w.shape[0])
                if i < 2:
                    gz = np.where((_np(acts[i]) > 0)[None], gz, 0.0)
                gz = gz.reshape(g.shape[0], -1)
                ref_gx = (_bf16(gz) @ _bf16(_np(w))) if math_mode == "bf16" else gz @ _np(w)
                ref_gx = np.where(np.tile(_np(xin) > 0, (g.shape[0] // B, 1)), ref_gx, 0.0)
                _close(_np(gx), ref_gx, tol_gx, f"g_x{i} b{B}")
                # the same device code as bnn_laplace_layer: the same bits on the same inputs
                gx_diag = torch.full_like(gx, float("nan"))
                ops.laplace_layer(xin, g, w, f_w=torch.zeros_like(w), f_b=torch.zeros(w.shape[0], device=dev), g_x=gx_diag, y=ysv,
                                  gx_mask=True, math_mode=mm)
                assert torch.equal(gx.view(torch.int32), gx_diag.view(torch.int32))
                g = gx
    assert all(bool(torch.isfinite(t).all()) for t in fa + fs + fg)
    assert all(bool((torch.diagonal(t) >= 0).all()) for t in fa + fg)


# ------------------------------------------------------------------------------------------------------------ 2. end to end
@pytest.mark.parametrize("curvature", ["ggn", "empirical"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_two_minibatches_against_the_jacobian_reference(dev, case, curvature):
    """Bound (test_gpu_laplace's rule): 10 x the max-norm error (relative to each tensor's largest entry; the largest over the
    tensors) of the same chain in plain fp32 torch on the CPU against fp64, on the same inputs; the factor covers another
    summation order on the device.  No hidden pre-activation may lie within 8 x the fp32 forward's own error of zero."""
    mode, inp, hid, C, _ = case
    bnn_hip.set_math("f32")
    mlp = _mlp(dev, mode, inp, hid, C, seed=1)
    la = bnn_hip.KronLaplace(mlp, curvature=curvature, sigma=SIGMA)
    weights = _weights(mlp)
    xs, ys = [], []
    for bi, B in enumerate(_two_batches(case)):
        x, y = _batch(dev, mlp, B, seed=22 + bi)
        la.accumulate(x, y)
        xs.append(_np(x).reshape(B, -1))
        ys.append(y.cpu().numpy())
    margin, fwd_err = _relu_margin(weights, xs)
    assert margin > 8 * fwd_err, (margin, fwd_err)
    base, restated = K.fp32_chain_error(weights, xs, ys, mode, curvature, SIGMA)
    ref = K.jacobian_factors(weights, np.concatenate(xs), np.concatenate(ys), mode, curvature, SIGMA)
    for rl, jl in zip(restated, ref):
        for r, j in zip(rl, jl):
            assert np.abs(r - j).max() <= 1e-11 * np.abs(j).max()                     # the two fp64 forms agree
    print(f"{IDS[CASES.index(case)]} {curvature}: fp32 base error {base:.3e}, bound {10 * base:.3e}")
    assert 0 < base < 1e-5
    for l, (a, s, g) in enumerate(ref):
        _close(_np(la.A[l]), a, 10 * base, f"A{l}")
        _close(_np(la.s[l]), s, 10 * base, f"s{l}")
        _close(_np(la.G[l]), g, 10 * base, f"G{l}")
    assert la.n_rows == sum(_two_batches(case))


# ------------------------------------------------------------------------------------------------------------ 3. accumulation
def test_accumulation_is_deterministic_and_reset_zeroes(dev):
    bnn_hip.set_math("f32")
    mode, inp, hid, C, batches = CASES[0]
    mlp = _mlp(dev, mode, inp, hid, C)
    data = [_batch(dev, mlp, B, seed=30 + i) for i, B in enumerate(batches)]
    runs = []
    for _ in range(2):
        la = mlp.laplace(structure="kron")
        assert isinstance(la, bnn_hip.KronLaplace) and isinstance(mlp.laplace(), bnn_hip.DiagLaplace)
        for x, y in data:
            la.accumulate(x, y)
        runs.append(_bits(la))
    assert _same(*runs) and all(bool((t != 0).any()) for t in runs[0])
    one = mlp.laplace(structure="kron")
    one.accumulate(*data[0])
    assert not _same(_bits(one), runs[0])                                  # the second minibatch did add something
    la.decompose()
    assert la._decomposed
    la.reset()
    assert all(bool((t == 0).all()) for t in _bits(la)) and not la._decomposed
    with pytest.raises(BnnHipError, match="nothing accumulated"):
        la.decompose()
    for x, y in data:
        la.accumulate(x, y)
    assert _same(_bits(la), runs[0])


@pytest.mark.parametrize("case", CASES[:2], ids=IDS[:2])
def test_graph_replays_equal_eager_launches_bit_for_bit(dev, case):
    bnn_hip.set_math("f32")
    mode, inp, hid, C, batches = case
    B = batches[0]
    mlp = _mlp(dev, mode, inp, hid, C)
    data = [_batch(dev, mlp, B, seed=40 + i) for i in range(5)]
    eager, graphed = mlp.laplace(structure="kron", sigma=SIGMA), mlp.laplace(structure="kron", sigma=SIGMA)
    step = graphed.accumulate_graph(*data[0])
    assert all(bool((t == 0).all()) for t in _bits(graphed))               # building the step accumulates nothing
    for x, y in data:
        eager.accumulate(x, y)
        step.step(x, y)
    assert _same(_bits(eager), _bits(graphed)) and eager.n_rows == 5 * B
    assert graphed.accumulate_graph(*data[0])._chain is step._chain        # one capture per batch size
    graphed.decompose()
    step.step(*data[0])
    assert not graphed._decomposed                                         # a replay invalidates the eigenbasis too


def test_fit_twice_gives_the_same_bits(dev):
    bnn_hip.set_math("f32")
    mode, inp, hid, C, batches = CASES[0]
    mlp = _mlp(dev, mode, inp, hid, C)
    loader = [_batch(dev, mlp, B, seed=50 + i) for i, B in enumerate((33, 33, 1))]
    la = mlp.laplace(structure="kron", curvature="empirical")
    first = _bits(la.fit(loader))
    assert la.n_rows == 67
    assert _same(first, _bits(la.fit(loader)))


# ------------------------------------------------------------------------------------------------------------ fitted posteriors
_FITTED = {}


def _fitted(dev, ci):
    """One fitted posterior per case (f32 math), shared by the read-only tests below: (mlp, la, data, x_test)."""
    if ci not in _FITTED:
        bnn_hip.set_math("f32")
        mode, inp, hid, C, batches = CASES[ci]
        mlp = _mlp(dev, mode, inp, hid, C, seed=2)
        data = [_batch(dev, mlp, B, seed=60 + i) for i, B in enumerate(_two_batches(CASES[ci]) * 2)]
        la = mlp.laplace(structure="kron", sigma=SIGMA).fit(data)
        xt = _batch(dev, mlp, 9, seed=77)
        _FITTED[ci] = (mlp, la, data, xt)
    bnn_hip.set_math("f32")
    return _FITTED[ci]


def _host_decomposition(la):
    """numpy's own fp64 eigh of the device's factors: [(Q_A, lA, Q_G, lG) per layer]."""
    N = la.n_rows
    return [K.decompose(_np(a), _np(s), _np(g), N) for a, s, g in zip(la.A, la.s, la.G)]


# ------------------------------------------------------------------------------------------------------------ 4. evidence
@pytest.mark.parametrize("ci", range(3), ids=IDS)
def test_log_evidence_and_the_chosen_precision(dev, ci):
    """Reference: the restated evidence with numpy's fp64 eigh of the device's own factors.  Two eigensolvers agree to about
    n eps |M| per eigenvalue, and d log(lG lA + tau) <= |d(lG lA)| / tau; with |lG||lA| the largest product of a layer that is
    a bound of P n eps max(lG lA) / tau on the sum -- added, with a factor 8 for the solver's constant, to the fp64 summation
    bound test_gpu_laplace uses."""
    mlp, la, _, _ = _fitted(dev, ci)
    taus = np.logspace(-4, 4, 9)
    got = la.log_evidence(taus)
    assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == (9,)
    decs = _host_decomposition(la)
    weights = _weights(mlp)
    rec = la.record.cpu().numpy()
    ref = K.evidence(weights, [(d[1], d[3]) for d in decs], taus, rec[0])
    w2 = sum((w ** 2).sum() + (b ** 2).sum() for w, b in weights)
    P = sum(w.size + b.size for w, b in weights)
    eps = 2.0 ** -53
    for g, (t, r) in enumerate(zip(taus, ref)):
        mag = sum(0.5 * np.abs(np.log(np.outer(d[3], d[1]) + t)).sum() for d in decs) + 0.5 * t * w2 + abs(0.5 * P * math.log(t)) + abs(rec[0])
        solver = sum(8 * d[1].size * d[3].size * max(d[1].size, d[3].size) * eps * d[1].max() * d[3].max() / t for d in decs)
        print(f"tau {t:g}: got {got[g].item():.12e} ref {r:.12e} diff {abs(got[g].item() - r):.3e} bound {1e-12 * abs(r) + P * eps * mag + solver:.3e}")
        assert abs(got[g].item() - r) <= 1e-12 * abs(r) + P * eps * mag + solver, (g, got[g].item(), r)
    best, gap = R.best_precision(ref)
    again = la.fit_prior_precision(taus)
    assert torch.equal(again, got)
    if gap > 1e-9:                                                          # the index cannot hinge on the summation order
        assert int(la._best_index.item()) == best == int(np.argmax(ref))
        assert la.prior_precision == taus[best]
    assert int(la._best_index.item()) == int(torch.argmax(got).item()) and la._best[0].item() == got.max().item()
    full = la.fit_prior_precision()                                         # the default grid: 33 candidates in one pass
    assert tuple(full.shape) == (33,) and bool(torch.isfinite(full).all())
    assert la.prior_precision == np.logspace(-4, 4, 33)[int(torch.argmax(full).item())]
    with pytest.raises(BnnHipError):
        la.log_evidence(np.logspace(-4, 4, L.LAPLACE_MAX_PRECISIONS + 1))
    # the device's own decomposition: orthonormal to fp32 rounding, eigenvalues clamped at 0, fp32 copies of the fp64 ones
    for l in range(len(la.layers)):
        for Q, lam, lam32 in ((la.Q_A[l], la.lam_A[l], la.lam_A32[l]), (la.Q_G[l], la.lam_G[l], la.lam_G32[l])):
            q = _np(Q)
            assert np.abs(q.T @ q - np.eye(q.shape[0])).max() <= 4e-6
            assert bool((lam >= 0).all()) and lam.dtype == torch.float64 and torch.equal(lam32, lam.float())


# ------------------------------------------------------------------------------------------------------------ 5. GLM moments
def _fp32_basis_floor(weights, xs, decs, tau, ref_cov):
    """The error (max-norm, relative to the largest covariance entry) of the fp64 restatement run with its eigenvectors rounded
    to fp32: the floor any fp32 basis has."""
    r32 = [(d[0].astype(np.float32).astype(np.float64), d[1], d[2].astype(np.float32).astype(np.float64), d[3]) for d in decs]
    return float(np.abs(K.glm_cov(weights, xs, r32, tau)[1] - ref_cov).max() / np.abs(ref_cov).max())


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("ci", range(3), ids=IDS)
def test_glm_moments_against_the_dense_precision(dev, ci, tau):
    """cov = J P^-1 J^T, basis-invariant: eigenvector signs and degenerate subspaces do not matter.  Reference at every shape:
    the dense fp64 kron(G, Abar) / N + tau I of the device's own factors (projected onto the positive semi-definite matrices,
    as the posterior is defined) and autograd Jacobians; at 119-100-10, where layer
    1's precision is 12 000 x 12 000, the fp64 LU runs on the device (torch.linalg.solve: the vendor's solver, none of the code
    under test).
    Tolerance: test_gpu_glm's rule for its covariance in f32 math -- 10 x the max-norm error (relative to the largest
    covariance entry) of the same eigenbasis formula in plain fp32 torch on the CPU against the reference, on the same inputs;
    the factor covers another summation order on the device.  The fp32-basis floor (the fp64 restatement with its eigenvectors
    rounded to fp32) is printed beside it (DESIGN.md F20 records both)."""
    mlp, la, _, (xt, _) = _fitted(dev, ci)
    weights, N = _weights(mlp), la.n_rows
    xs = _np(xt).reshape(xt.shape[0], -1)
    margin, fwd_err = _relu_margin(weights, [xs])
    assert margin > 8 * fwd_err, (margin, fwd_err)
    decs = _host_decomposition(la)
    ref_mean, restated = K.glm_cov(weights, xs, decs, tau)
    factors = [(_np(a), _np(s), _np(g)) for a, s, g in zip(la.A, la.s, la.G)]
    # (clamp: fp32-accumulated factors carry rounding-sized negative eigenvalues -- the softmax GGN's G has an exact null
    # direction -- and F20 defines the posterior with them set to 0; left in, they move the covariance by up to 4e-5 at tau = 1e-2)
    ref = K.dense_glm_cov(weights, xs, factors, N, tau, device=dev if ci == 2 else None, clamp=True)
    print(f"fp64 forms: rel diff {np.abs(restated - ref).max() / np.abs(ref).max():.3e}")
    assert np.abs(restated - ref).max() <= 1e-8 * np.abs(ref).max()                    # the two fp64 forms agree
    floor = _fp32_basis_floor(weights, xs, decs, tau, ref)
    base = float(np.abs(K.glm_cov_torch32(weights, xs, decs, tau).double().numpy() - ref).max() / np.abs(ref).max())
    print(f"{IDS[ci]} tau {tau:g}: fp32 base error {base:.3e}, bound {10 * base:.3e}, fp32-basis floor {floor:.3e}")
    assert 0 < base < 1e-5
    mean, cov = la.glm_moments(xt, prior_precision=tau)
    C = CASES[ci][3]
    assert tuple(mean.shape) == (9, C) and tuple(cov.shape) == (9, C, C)
    _close(_np(cov), ref, 10 * base, "cov")
    _close(_np(mean), ref_mean, 1e-5, "mean")
    assert np.linalg.eigvalsh(_np(cov)).min() > 0


@pytest.mark.parametrize("ci", range(3), ids=IDS)
def test_glm_stages_against_their_restatement(dev, ci):
    """bnn_kfac_glm_rotate and bnn_kfac_glm_var of the top hidden layer, from the kernels' own inputs and the device's own
    (Q, lambda): f32 max-norm 1e-5."""
    mlp, la, _, (xt, _) = _fitted(dev, ci)
    la.decompose()
    lins = [m for m in mlp.net if hasattr(m, "weight")]
    B, C, tau = xt.shape[0], CASES[ci][3], 0.5
    h = xt.reshape(B, -1).contiguous()
    acts = []
    for i, m in enumerate(lins):
        h = ops.dense_fwd(h, m.weight.detach(), m.bias.detach(), n_samples=1, math_mode=L.MATH_F32, relu=i < 2, drop_p=0.0,
                          layer_id=i, seed=0, y_dtype=torch.float32)[0]
        acts.append(h)
    g = torch.randn((B * C, lins[1].out_features), generator=torch.Generator().manual_seed(5)).to(dev)
    w = lins[1].weight.detach()
    gx = torch.full((B * C, w.shape[1]), float("nan"), device=dev)
    at, gt = ops.kfac_glm_rotate(acts[0], g, w, q_a=la.Q_A[1], q_g=la.Q_G[1], g_x=gx, y=acts[1], gx_mask=True)
    v = torch.full((B, w.shape[0]), float("nan"), device=dev)
    part = ops.kfac_glm_var(at, gt, la.lam_A[1], la.lam_G[1], v_out=v, precision=tau)
    word = torch.tensor([tau], dtype=torch.float64, device=dev)
    part2 = ops.kfac_glm_var(at, gt, la.lam_A[1], la.lam_G[1], precision_device=word)
    assert torch.equal(part.view(torch.int32), part2.view(torch.int32))                # the device word gives the same bits
    r_at, r_gt, r_v, r_cov = K.glm_layer(_np(acts[0]), _np(g), _np(acts[1]), _np(la.Q_A[1]), _np(la.lam_A[1]), _np(la.Q_G[1]),
                                         _np(la.lam_G[1]), tau)
    _close(_np(at), r_at, 1e-5, "at")
    _close(_np(gt), r_gt, 1e-5, "gt")
    _close(_np(v), r_v, 1e-5, "V")
    # the partials from the kernel's own at, gt: V and the pair sums
    k_v = _np(at) ** 2 @ (1.0 / (np.outer(_np(la.lam_G[1]), _np(la.lam_A[1])) + tau)).T
    _close(_np(v), k_v, 1e-5, "V from the kernel's at")
    g3 = _np(gt).reshape(C, B, -1)
    pairs = np.stack([np.einsum("nj,nj,nj->n", g3[ca], g3[cb], _np(v)) for cb in range(C) for ca in range(cb + 1)], axis=1)
    assert tuple(part.shape) == (ops.glm_tiles(w.shape[0]), B, C * (C + 1) // 2)
    _close(_np(part).sum(axis=0), pairs, 1e-5, "pair sums")
    full = np.stack([r_cov[:, ca, cb] for cb in range(C) for ca in range(cb + 1)], axis=1)
    _close(_np(part).sum(axis=0), full, 1e-5, "pair sums (restated)")
    gx_diag = torch.full_like(gx, float("nan"))
    ops.laplace_layer(acts[0], g, w, f_w=torch.zeros_like(w), f_b=torch.zeros(w.shape[0], device=dev), g_x=gx_diag, y=acts[1], gx_mask=True)
    assert torch.equal(gx.view(torch.int32), gx_diag.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------ 6. GLM predictive
def test_glm_predictive_fields_graph_replay_and_score(dev):
    mlp, la, data, (xt, yt) = _fitted(dev, 0)
    la.fit_prior_precision()
    p = la.glm_predictive(xt)
    assert tuple(p.probs.shape) == (9, 3) and tuple(p.preds.shape) == (9,) and tuple(p.predictive_entropy.shape) == (9,)
    assert p.expected_entropy is None and p.mutual_information is None
    np.testing.assert_allclose(_np(p.probs).sum(axis=1), 1.0, atol=1e-6)
    m = la.glm_predictive(xt, 16, link="mc", sample_offset=1000)
    for f in (m.probs, m.preds, m.predictive_entropy, m.expected_entropy, m.mutual_information):
        assert f is not None and bool(torch.isfinite(f.float()).all())
    again = la.glm_predictive(xt, 16, link="mc", sample_offset=1000)
    assert torch.equal(m.probs, again.probs) and torch.equal(m.mutual_information, again.mutual_information)
    for link in ("probit", "mc"):
        bnn_hip.manual_seed(2026)
        g = la.glm_predictive_graph(xt, 16, link=link)
        c0 = int(g.counter.item()) & 0xFFFFFFFF
        r = g.replay()
        c1 = int(g.counter.item()) & 0xFFFFFFFF
        eager = la.glm_predictive(xt, 16, link=link, sample_offset=c1 - 16 if link == "mc" else None)
        assert torch.equal(r.probs, eager.probs) and torch.equal(r.preds, eager.preds)
        assert torch.equal(r.predictive_entropy, eager.predictive_entropy)
        assert c1 - c0 == (16 if link == "mc" else 0)
    sc = la.glm_score(xt, yt, 16).read()
    assert sc.n == 9 and math.isfinite(sc.lpd) and math.isfinite(sc.nll) and math.isfinite(sc.brier)
    s = la.glm_sample(xt, 4, sample_offset=3)
    assert tuple(s.shape) == (4, 9, 3) and bool(torch.isfinite(s).all())
    # regression: closed-form fields, quantiles, and the score
    rm, rla, _, (rx, ry) = _fitted(dev, 1)
    r = rla.glm_predictive(rx, quantiles=[0.025, 0.5, 0.975], sigma=0.5)
    np.testing.assert_allclose(_np(r.predictive_variance), _np(r.variance) + 0.25, rtol=1e-6)
    np.testing.assert_allclose(_np(r.quantiles[1]), _np(r.mean), rtol=1e-6, atol=1e-7)
    assert bool((r.variance > 0).all())
    rs = rla.glm_score(rx, ry, 8).read()
    assert rs.n == 9 and math.isfinite(rs.lpd)


# ------------------------------------------------------------------------------------------------------------ 7. sample_bank
@pytest.mark.parametrize("ci", range(3), ids=IDS)
def test_sample_bank_against_the_restated_stream(dev, ci):
    """Members against Wbar + Q_G (E o Sigma) Q_A^T with E from the oracle's Philox / Box-Muller and the device's own (Q, lambda),
    in the f32 max-norm tolerance 1e-5 x the largest |entry| of the member.
    Printed beside it, measured without the kernel under test: what the device's fast Box-Muller alone moves a member by --
    the difference between the device's materialised SG-MCMC noise (bnn_sgmcmc_noise: the same device Box-Muller) and its
    oracle restatement, as many values as the layer has, carried through the fp64 map."""
    import sgmcmc_ref
    mlp, la, _, _ = _fitted(dev, ci)
    tau, seed, off = 0.7, 2026, 40
    bnn_hip.manual_seed(seed)
    bank = la.sample_bank(3, sample_offset=off, prior_precision=tau)
    assert isinstance(bank, bnn_hip.WeightBank) and bank.count() == 3
    la.decompose()
    for l, (w, b) in enumerate(_weights(mlp)):
        QA, lA, QG, lG = (_np(t) for t in (la.Q_A[l], la.lam_A[l], la.Q_G[l], la.lam_G[l]))
        n = w.shape[0] * (w.shape[1] + 1)
        d = _np(ops.sgmcmc_noise(seed, l, off, n, dev)) - sgmcmc_ref.noise(seed, l, off, n).astype(np.float64)
        moved = QG @ (d.reshape(w.shape[0], -1) * (np.outer(lG, lA) + tau) ** -0.5) @ QA.T
        for m in (0, 2):
            E = K.noise(seed, off + m, l, w.shape[0], w.shape[1] + 1)
            ws, bs = K.sample(w, b, QA, lA, QG, lG, tau, E)
            vw, vb = bank.views(m)[2 * l], bank.views(m)[2 * l + 1]
            ref = np.concatenate([ws, bs[:, None]], axis=1)
            got = np.concatenate([_np(vw), _np(vb)[:, None]], axis=1)
            print(f"{IDS[ci]} layer {l} member {m}: Box-Muller alone {np.abs(moved).max() / np.abs(ref).max():.3e} of the largest entry "
                  f"(noise difference at most {np.abs(d).max():.3e})")
            _close(got, ref, 1e-5, f"member {m} layer {l}")
            assert np.abs(got - np.concatenate([w, b[:, None]], axis=1)).max() > 0      # a draw, not the mean


def test_sample_bank_offsets_chunks_and_the_bank_tools(dev):
    mlp, la, data, (xt, yt) = _fitted(dev, 0)
    la.fit_prior_precision()
    bnn_hip.manual_seed(7)
    a = la.sample_bank(5, sample_offset=11)
    b = la.sample_bank(5, sample_offset=11, budget_bytes=1)                 # one member per launch
    assert la.members_per_launch(5, 1) == 1 and la.members_per_launch(5) == 5
    assert torch.equal(a.buffer.view(torch.int32), b.buffer.view(torch.int32))           # chunked = unchunked, bit for bit
    c = la.sample_bank(5, bank=b, sample_offset=12)
    assert c is b and not torch.equal(a.buffer, b.buffer)
    assert torch.equal(a.views(1)[0], b.views(0)[0])                        # global sample 12 is the same draw in either slot
    d = la.sample_bank(2)                                                   # the process-wide counter by default
    e = la.sample_bank(2)
    assert not torch.equal(d.buffer, e.buffer)
    with pytest.raises(BnnHipError, match="must hold 5 members"):
        la.sample_bank(5, bank=d)
    p = a.predictive(xt)
    for f in (p.probs, p.preds, p.predictive_entropy, p.expected_entropy, p.mutual_information):
        assert f is not None and bool(torch.isfinite(f.float()).all())
    assert tuple(p.probs.shape) == (9, 3)
    preds, probs = a.predict_mc(xt)
    assert tuple(probs.shape) == (9, 3) and tuple(preds.shape) == (9,)
    sc = a.score(xt, yt).read()
    assert sc.n == 9 and math.isfinite(sc.lpd) and math.isfinite(sc.brier)
    assert not hasattr(la, "network")


# ------------------------------------------------------------------------------------------------------------ 8. failure modes
@pytest.mark.parametrize("curvature", ["ggn", "empirical"])
def test_out_of_range_label_gives_nan_and_no_fault(dev, curvature):
    bnn_hip.set_math("f32")
    mode, inp, hid, C, _ = CASES[0]
    mlp = _mlp(dev, mode, inp, hid, C)
    x, y = _batch(dev, mlp, 5, seed=70)
    y = y.clone()
    y[2] = C                                                                # one past the last class
    y[4] = -1
    la = mlp.laplace(structure="kron", curvature=curvature)
    la.accumulate(x, y)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).any()) for t in la.G) and math.isnan(la.record[0].item()) and la.n_rows == 5
    assert all(bool(torch.isfinite(t).all()) for t in la.A + la.s)         # the inputs' factor does not see the labels


def test_c_abi_error_codes_come_back_in_the_documented_order(dev):
    """The refusals of the five entry points, status by status in the header's order, on the machine with the device too (the
    cases are tests/test_kfac_cpu.py's: a refused call never reaches its stream or its pointers)."""
    import test_kfac_cpu as cpu
    cpu.test_kfac_layer_argument_errors()
    cpu.test_kfac_evidence_argument_errors()
    cpu.test_kfac_glm_argument_errors()
    cpu.test_kfac_sample_argument_errors()


def test_a_captured_predictive_follows_a_refit(dev):
    """A replay after more data has been accumulated reads the new eigenbasis: the same bits as an eager call then."""
    mode, inp, hid, C, _ = CASES[0]
    bnn_hip.set_math("f32")
    mlp = _mlp(dev, mode, inp, hid, C, seed=3)
    data = [_batch(dev, mlp, 33, seed=90 + i) for i in range(3)]
    la = mlp.laplace(structure="kron").fit(data[:2])
    xt, _ = _batch(dev, mlp, 9, seed=95)
    g = la.glm_predictive_graph(xt, link="probit", prior_precision=1.0)
    before = g.replay().probs.clone()
    la.accumulate(*data[2])
    assert not la._decomposed
    after = g.replay().probs.clone()
    assert la._decomposed and not torch.equal(before, after)
    assert torch.equal(after, la.glm_predictive(xt, prior_precision=1.0).probs)


def test_refusals_on_the_device(dev):
    import networks
    bnn_hip.set_math("f32")
    mode, inp, hid, C, _ = CASES[0]
    drop = _mlp(dev, mode, inp, hid, C, dropout=True)
    with pytest.raises(BnnHipError, match="dropout is on"):
        drop.laplace(structure="kron")
    drop.eval()
    plain = _mlp(dev, mode, inp, hid, C)
    plain.load_state_dict({k.replace("net.3", "net.2").replace("net.6", "net.4"): v for k, v in drop.state_dict().items()})
    x, y = _batch(dev, drop, 33, seed=80)
    a, b = drop.laplace(structure="kron"), plain.laplace(structure="kron")
    a.accumulate(x, y)
    b.accumulate(x, y)
    assert _same(_bits(a), _bits(b))                                        # the same weights, the same factors
    nobias = _mlp(dev, mode, inp, hid, C)
    nobias.net[0] = torch.nn.Linear(inp, hid, bias=False).to(dev)
    with pytest.raises(BnnHipError, match="needs a bias"):
        nobias.laplace(structure="kron")
    bnn_hip.shard_samples(True)
    try:
        with pytest.raises(BnnHipError, match="sharding is not supported"):
            plain.laplace(structure="kron")
    finally:
        bnn_hip.shard_samples(False)
    bnn_hip.set_math("bf16")
    with pytest.raises(BnnHipError, match="math mode changed"):
        b.accumulate(x, y)
    with pytest.raises(BnnHipError, match="math mode changed"):
        b.sample_bank(2)
    bnn_hip.set_math("f32")
    wide = _mlp(dev, mode, inp, hid, 17).laplace(structure="kron")
    with pytest.raises(BnnHipError, match="at most 16 outputs"):
        wide.glm_moments(x)
