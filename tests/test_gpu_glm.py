"""The linearised (GLM) predictive of the diagonal Laplace posterior on the device (bnn_laplace_glm_layer / _finish / _sample,
DiagLaplace.glm_*; include/bnn_hip.h F18): every stage against its fp64 restatement (tests/glm_ref.py) computed from the
kernel's own inputs, the finish from the device's own partials, the moments end to end against J diag(s^2) J^T from autograd
Jacobians, the sampler against the restated Philox stream, the 'mc' route against bnn_mc_predictive / bnn_mc_score by hand,
determinism, graph replays, untouched state, and a NaN curvature entry.

Shapes: test_gpu_laplace.py's (every edge of a 64-tile and of a 32-wide k stage) -- 70-65-3 with batches 33 and 1, 1-40-1 with
batch 5, 119-100-10 with batch 64 -- plus 20-24-16 with batch 3, the class limit.  F comes from a real two-minibatch fit in f32
math; tau = 1."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bnn_hip
import glm_ref as G
from bnn_hip import _lib as L
from bnn_hip import ops
from bnn_hip.engine import _first_minibatch
from bnn_hip.ops import BnnHipError
from bnn_hip.runtime import state
from test_gpu_laplace import SIGMA, _batch, _bf16, _close, _mlp, _np, _relu_margin, _weights

#        mode, input, hidden, classes, batch, the two minibatches of the fit
CASES = [("classification", 70, 65, 3, 33, (33, 1)),
         ("classification", 70, 65, 3, 1, (33, 1)),
         ("regression", 1, 40, 1, 5, (5, 5)),
         ("classification", 119, 100, 10, 64, (64, 64)),
         ("classification", 20, 24, 16, 3, (3, 3))]
IDS = ["70-65-3-b33", "70-65-3-b1", "1-40-1-b5", "119-100-10-b64", "20-24-16-b3"]
TAU = 1.0
LEVELS = (0.0, 0.05, 0.5, 0.95, 1.0)
U = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore():
    yield
    bnn_hip.set_math("bf16")
    bnn_hip.manual_seed(2026)


_fits, _runs = {}, {}


def _fitted(dev, case, curvature="ggn"):
    """(mlp, la, x): a posterior fitted on two minibatches in f32 math (built once per case and never written) and the batch
    the predictive is asked for."""
    key = (IDS[CASES.index(case)], curvature)
    if key not in _fits:
        mode, inp, hid, C, B, fit = case
        bnn_hip.set_math("f32")
        mlp = _mlp(dev, mode, inp, hid, C, seed=3)
        la = mlp.laplace(curvature=curvature, sigma=SIGMA).fit([_batch(dev, mlp, b, seed=90 + i) for i, b in enumerate(fit)])
        x, y = _batch(dev, mlp, B, seed=95)
        _fits[key] = (mlp, la, x, y)
    return _fits[key]


def _bits(ts):
    return [t.clone() for t in ts]


def _same(a, b):
    return len(a) == len(b) and all((s is None and t is None) or torch.equal(s.contiguous().view(torch.uint8), t.contiguous().view(torch.uint8))
                                    for s, t in zip(a, b))


def _stages(dev, case, math_mode):
    """One run of the launches by hand (exact-fp32 forward, as test_gpu_laplace does, so that every later stage sees the same
    inputs in both math modes), everything kept: shared by the stage, finish and sampler tests."""
    key = (IDS[CASES.index(case)], math_mode)
    if key in _runs:
        return _runs[key]
    mode, inp, hid, C, B, _ = case
    mlp, la, x, _ = _fitted(dev, case)
    bnn_hip.set_math(math_mode)
    mm = L.MATH_BF16 if math_mode == "bf16" else L.MATH_F32
    lins = [m for m in mlp.net if hasattr(m, "weight")]
    xf = x.reshape(B, -1).contiguous()
    acts, h = [], xf
    for i, m in enumerate(lins):
        h = ops.dense_fwd(h, m.weight.detach(), m.bias.detach(), n_samples=1, math_mode=L.MATH_F32, relu=i < 2, drop_p=0.0,
                          layer_id=i, seed=0, y_dtype=torch.float32)[0]
        acts.append(h)
    scratch = torch.zeros(2, dtype=torch.float64, device=dev)
    gy = ops.laplace_seed(acts[-1], None, "regression", curvature="ggn", sigma=1.0, record=scratch)
    assert torch.equal(gy.reshape(C, B, C), torch.eye(C, device=dev)[:, None, :].expand(C, B, C)) and scratch.tolist() == [0.0, B]
    run = dict(xf=xf, acts=acts, gy=gy, layers=[None] * 3, mm=mm)
    g = gy
    for i in (2, 1, 0):
        xin = xf if i == 0 else acts[i - 1]
        w = lins[i].weight.detach()
        v_out = torch.full((B, w.shape[0]), float("nan"), device=dev)
        gx = torch.full((g.shape[0], w.shape[1]), float("nan"), device=dev) if i > 0 else None
        part = torch.full((ops.glm_tiles(w.shape[0]), B, ops.glm_pairs(C)), float("nan"), device=dev)
        got = ops.laplace_glm_layer(xin, g, w, f_w=la.curv[2 * i], f_b=la.curv[2 * i + 1], cov_part=part, g_x=gx,
                                    y=acts[i] if i < 2 else None, gx_mask=i > 0, v_out=v_out, precision=TAU, math_mode=mm)
        assert got is part
        run["layers"][i] = dict(xin=xin, g=g, w=w, v=v_out, gx=gx, part=part, y=acts[i] if i < 2 else None)
        g = gx
    _runs[key] = run
    return run


# ------------------------------------------------------------------------------------------------------------ 1. stage by stage
@pytest.mark.parametrize("math_mode,tol_gx", [("f32", 1e-5), ("bf16", 2e-3)])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_stage_against_its_fp64_restatement(dev, case, math_mode, tol_gx):
    """V and the summed partials (always exact fp32) at max-norm 1e-5, g_x at F17's 1e-5 / 2e-3; g_x is also bit for bit what
    bnn_laplace_layer writes for the same inputs (one device function)."""
    mode, inp, hid, C, B, _ = case
    _, la, _, _ = _fitted(dev, case)
    run = _stages(dev, case, math_mode)
    for i in (2, 1, 0):
        s = run["layers"][i]
        tag = f"L{i} {math_mode}"
        V = G.v_of(_np(s["xin"]), _np(la.curv[2 * i]), _np(la.curv[2 * i + 1]), TAU)
        assert bool(torch.isfinite(s["v"]).all()) and bool(torch.isfinite(s["part"]).all())
        _close(_np(s["v"]), V, 1e-5, f"V {tag}")
        y = None if s["y"] is None else _np(s["y"])
        got = _np(s["part"]).sum(axis=0)
        assert s["part"].shape == (ops.glm_tiles(s["w"].shape[0]), B, C * (C + 1) // 2)
        _close(got, G.layer_parts(_np(s["g"]), y, _np(s["v"]), B).sum(axis=0), 1e-5, f"partials from the kernel's V {tag}")
        _close(got, G.layer_parts(_np(s["g"]), y, V, B).sum(axis=0), 1e-5, f"partials from the restated V {tag}")
        _close(_np(s["part"]), G.layer_parts(_np(s["g"]), y, _np(s["v"]), B), 1e-5, f"each tile {tag}")
        if i > 0:
            gz = _np(s["g"]).reshape(C, B, -1)
            if y is not None:
                gz = np.where((y > 0)[None], gz, 0.0)
            gz = gz.reshape(C * B, -1)
            ref = (_bf16(gz) @ _bf16(_np(s["w"]))) if math_mode == "bf16" else gz @ _np(s["w"])
            ref = np.where(np.tile(_np(s["xin"]) > 0, (C, 1)), ref, 0.0)
            _close(_np(s["gx"]), ref, tol_gx, f"g_x {tag}")
            fw, fb = torch.zeros_like(la.curv[2 * i]), torch.zeros_like(la.curv[2 * i + 1])
            gx17 = torch.full_like(s["gx"], float("nan"))
            ops.laplace_layer(s["xin"], s["g"], s["w"], f_w=fw, f_b=fb, g_x=gx17, y=s["y"], gx_mask=True, math_mode=run["mm"])
            assert _same([gx17], [s["gx"]])


# ------------------------------------------------------------------------------------------------------------ 2. finish
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_finish_from_the_devices_own_partials(dev, case):
    mode, inp, hid, C, B, _ = case
    run = _stages(dev, case, "f32")
    parts = [s["part"] for s in run["layers"]]
    mean = run["acts"][-1]
    levels = LEVELS if mode == "regression" else ()
    m = ops.laplace_glm_finish(parts, mean, mode, sigma=SIGMA, quantiles=levels)
    ref = G.finish([_np(p) for p in parts], _np(mean), mode, SIGMA, levels)
    cov, var, chol = _np(m.cov), _np(m.var), _np(m.chol)
    assert np.isfinite(cov).all() and (cov == cov.transpose(0, 2, 1)).all()
    rel = np.abs(cov - ref["cov"]) / np.abs(ref["cov"]).clip(1e-300)
    print(f"cov: max rel err {rel.max():.3e} (2^-23 = {2 * U:.3e}); var min {var.min():.3e}")
    assert (np.abs(cov - ref["cov"]) <= 2 * U * np.abs(ref["cov"])).all()
    assert (np.abs(var - ref["var"]) <= 2 * U * np.abs(ref["var"])).all() and (var == np.einsum("ncc->nc", cov)).all()
    assert (np.triu(chol, 1) == 0).all() and (np.einsum("ncc->nc", chol) > 0).all()
    resid = np.abs(chol @ chol.transpose(0, 2, 1) - cov)
    bound = (C + 2) * U * (np.abs(chol) @ np.abs(chol).transpose(0, 2, 1))
    print(f"chol: max resid / bound {(resid / bound).max():.3f}")
    assert (resid <= bound).all()
    _close(chol, ref["chol"], 1e-5, "chol against fp64")
    if mode == "classification":
        assert m.predictive_variance is None and m.quantiles is None
        np.testing.assert_allclose(_np(m.probs), ref["probs"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(_np(m.entropy), ref["entropy"], rtol=1e-5, atol=1e-5)
        preds = m.preds.cpu().numpy()
        assert m.preds.dtype == torch.int64 and (preds == np.argmax(m.probs.cpu().numpy(), axis=1)).all()
        top = np.sort(ref["probs"], axis=1)
        clear = (top[:, -1] - top[:, -2] > 4e-6) if C > 1 else np.ones(B, dtype=bool)
        assert clear.any() and (preds[clear] == ref["preds"][clear]).all()
    else:
        assert m.probs is None and m.preds is None and m.entropy is None
        np.testing.assert_allclose(_np(m.predictive_variance), ref["predictive_variance"], rtol=1e-6)
        q = _np(m.quantiles)
        assert q.shape == (len(LEVELS), B, C) and (q[0] == -np.inf).all() and (q[-1] == np.inf).all()
        np.testing.assert_allclose(q[1:-1], ref["quantiles"][1:-1], rtol=1e-6)


# ------------------------------------------------------------------------------------------------------------ 3. end to end
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_moments_end_to_end_against_the_jacobian_reference(dev, case):
    """f32 math.  Bound: 10 x the max-norm error (relative to the largest covariance entry) of the same layer-wise formula in
    plain fp32 torch on the CPU against fp64, on the same inputs; the factor covers another summation order on the device.  No
    hidden pre-activation may lie within 8 x the fp32 forward's own error of zero (asserted first).
    Measured base errors (fp32 CPU against fp64): see DESIGN.md F18."""
    mode, inp, hid, C, B, _ = case
    mlp, la, x, _ = _fitted(dev, case)
    bnn_hip.set_math("f32")
    weights = _weights(mlp)
    xs = _np(x).reshape(B, -1)
    margin, fwd_err = _relu_margin(weights, [xs])
    assert margin > 8 * fwd_err, (margin, fwd_err)
    curv = [_np(t) for t in la.curv]
    ref_mean, ref_cov = G.jacobian_cov(weights, curv, TAU, xs)
    _, restated, _ = G.chain(weights, curv, TAU, xs)
    assert np.abs(restated - ref_cov).max() <= 1e-10 * np.abs(ref_cov).max()          # the two fp64 forms agree
    base = float(np.abs(G.chain_torch32(weights, curv, TAU, xs).double().numpy() - ref_cov).max() / np.abs(ref_cov).max())
    print(f"{IDS[CASES.index(case)]}: fp32 base error {base:.3e}, bound {10 * base:.3e}")
    assert 0 < base < 1e-5
    mean, cov = la.glm_moments(x, prior_precision=TAU)
    assert tuple(mean.shape) == (B, C) and tuple(cov.shape) == (B, C, C)
    _close(_np(cov), ref_cov, 10 * base, "cov")
    _close(_np(mean), ref_mean, 1e-5, "mean")
    assert np.linalg.eigvalsh(_np(cov)).min() > 0


def test_an_empirical_fisher_object_is_accepted(dev):
    case = CASES[0]
    mlp, la, x, _ = _fitted(dev, case, curvature="empirical")
    bnn_hip.set_math("f32")
    mean, cov = la.glm_moments(x, prior_precision=TAU)
    _, ref, _ = G.chain(_weights(mlp), [_np(t) for t in la.curv], TAU, _np(x).reshape(case[4], -1))
    _close(_np(cov), ref, 1e-5, "cov (empirical Fisher)")


# ------------------------------------------------------------------------------------------------------------ 4. sampler
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_sampler_against_the_restated_stream(dev, case):
    """|f - ref| <= (C + 2) 2^-24 (|mean| + sum_j |chol_cj| |z_j|) from the device's own (mean, chol) and the restated eps."""
    mode, inp, hid, C, B, _ = case
    run = _stages(dev, case, "f32")
    mean = run["acts"][-1]
    m = ops.laplace_glm_finish([s["part"] for s in run["layers"]], mean, mode, sigma=SIGMA)
    S, seed, first = 7, 0x1234567887654321, 1000
    f = ops.laplace_glm_sample(mean, m.chol, S, seed=seed, sample_base=first)
    assert tuple(f.shape) == (S, B, C) and f.dtype == torch.float32
    ref, mag = G.sample(_np(mean), _np(m.chol), seed, first, S)
    ratio = np.abs(_np(f) - ref) / ((C + 2) * U * mag)
    print(f"sampler: max |f - ref| / bound = {ratio.max():.3f}")
    assert (ratio <= 1.0).all()
    # the counter: *counter - S is added to the base; a second call with the counter advanced by S equals sample_base + S
    counter = torch.tensor([S], dtype=torch.int32, device=dev)
    assert _same([ops.laplace_glm_sample(mean, m.chol, S, seed=seed, sample_base=first, sample_counter=counter)], [f])
    counter += S
    second = ops.laplace_glm_sample(mean, m.chol, S, seed=seed, sample_base=first, sample_counter=counter)
    assert _same([second], [ops.laplace_glm_sample(mean, m.chol, S, seed=seed, sample_base=first + S)]) and not _same([second], [f])
    assert _same([ops.laplace_glm_sample(mean, m.chol, 2 * S, seed=seed, sample_base=first)], [torch.cat([f, second])])
    assert not _same([ops.laplace_glm_sample(mean, m.chol, S, seed=seed + 1, sample_base=first)], [f])


def test_samples_do_not_depend_on_the_grid(dev):
    """Batch 33 (S = 7: one block) against the same rows inside a batch of 70 with S = 64 (eighteen blocks)."""
    case = CASES[0]
    run = _stages(dev, case, "f32")
    mean = run["acts"][-1]
    m = ops.laplace_glm_finish([s["part"] for s in run["layers"]], mean, case[0])
    g = torch.Generator().manual_seed(1)
    mean70 = torch.cat([mean, torch.randn((37, 3), generator=g).to(dev)])
    chol70 = torch.cat([m.chol, torch.tril(torch.randn((37, 3, 3), generator=g)).to(dev)]).contiguous()
    small = ops.laplace_glm_sample(mean, m.chol, 7, seed=5, sample_base=40)
    big = ops.laplace_glm_sample(mean70, chol70, 64, seed=5, sample_base=40)
    assert _same([big[:7, :33]], [small])


# ------------------------------------------------------------------------------------------------------------ 5. the mc route
@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[4]], ids=[IDS[0], IDS[2], IDS[4]])
def test_mc_predictive_and_score_equal_the_existing_kernels_by_hand(dev, case):
    mode, inp, hid, C, B, _ = case
    mlp, la, x, y = _fitted(dev, case)
    bnn_hip.set_math("f32")
    S, first = 16, 4000
    g = la.glm_predictive_graph(x, S, link="mc", prior_precision=TAU, capture=False)
    g.counter.fill_(first)
    r = g.replay()
    chol = g.moments.chol
    mean = g._chain.mean
    logits = ops.laplace_glm_sample(mean, chol, S, seed=state.seed, sample_base=first)
    assert _same([la.glm_sample(x, S, prior_precision=TAU, sample_offset=first)], [logits])
    eager = la.glm_predictive(x, S, link="mc", prior_precision=TAU, sample_offset=first)
    if mode == "classification":
        assert _same([g.logits], [logits]) and int(g.counter.item()) == first + S
        hand = _first_minibatch(ops.mc_predictive(logits, "classification"))
        assert all(t is not None for t in hand[:5]) and _same(list(hand), list(r)) and _same(list(hand), list(eager))
    else:                                                        # regression: closed form under either link, nothing sampled
        assert g.logits is None and int(g.counter.item()) == first
        probit = la.glm_predictive(x, prior_precision=TAU)
        assert _same(list(eager), list(probit)) and _same(list(eager), list(r)) and eager.probs is None
        assert _same([eager.mean], [mean]) and _same([eager.variance], [g.moments.var])
        np.testing.assert_allclose(_np(eager.predictive_variance), _np(eager.variance) + SIGMA ** 2, rtol=1e-6)
    sc = la.glm_score(x, y, S, prior_precision=TAU, sample_offset=first)
    hand_sc = ops.mc_score(logits, y, mode, sigma=SIGMA, bins=10)
    assert torch.equal(sc.record, hand_sc.record) and sc.read().n == B


# ------------------------------------------------------------------------------------------------------------ 6. determinism, state
def test_repeats_graph_replays_and_untouched_state(dev):
    case = CASES[0]
    mode, inp, hid, C, B, _ = case
    mlp, la, x, y = _fitted(dev, case)
    bnn_hip.set_math("f32")
    before = _bits(la.curv + [la.record])
    x2, _ = _batch(dev, mlp, B, seed=96)
    S = 16
    # the same call twice
    a, b = la.glm_moments(x, prior_precision=TAU), la.glm_moments(x, prior_precision=TAU)
    assert _same(list(a), list(b))
    p1 = la.glm_predictive(x, S, link="mc", prior_precision=TAU, sample_offset=7000)
    p2 = la.glm_predictive(x, S, link="mc", prior_precision=TAU, sample_offset=7000)
    assert _same(list(p1), list(p2))
    assert not _same(list(p1), list(la.glm_predictive(x, S, link="mc", prior_precision=TAU)))       # the process-wide counter moved on
    # probit: a captured graph against eager launches, on another input than the one it was captured with
    g = la.glm_predictive_graph(x, prior_precision=TAU)
    assert g.graph is not None and tuple(g.x.shape) == (B, inp)
    g.x.copy_(x2.reshape(B, -1))
    r = g.replay()
    e = la.glm_predictive(x2, prior_precision=TAU)
    assert r.expected_entropy is None and r.mutual_information is None and r.mean is None
    assert _same(list(r), list(e)) and not _same(list(e), list(la.glm_predictive(x, prior_precision=TAU)))
    # mc: the device counter gives every replay fresh samples; the same counter value gives the same bits as eager launches
    gm = la.glm_predictive_graph(x, S, link="mc", prior_precision=TAU)
    gm.counter.fill_(5000)
    r1 = [None if t is None else t.clone() for t in gm.replay()]
    assert int(gm.counter.item()) == 5000 + S
    r2 = [None if t is None else t.clone() for t in gm.replay()]
    assert _same(r1, list(la.glm_predictive(x, S, link="mc", prior_precision=TAU, sample_offset=5000)))
    assert _same(r2, list(la.glm_predictive(x, S, link="mc", prior_precision=TAU, sample_offset=5000 + S))) and not _same(r1, r2)
    # the default precision is the device word fit_prior_precision chose: the same bits as the host value
    d = la.glm_moments(x)
    assert _same(list(d), list(la.glm_moments(x, prior_precision=la.prior_precision)))
    la.glm_score(x, y, S)
    torch.cuda.synchronize()
    assert _same(before, _bits(la.curv + [la.record]))


def test_regression_graph_with_quantiles(dev):
    case = CASES[2]
    mlp, la, x, _ = _fitted(dev, case)
    bnn_hip.set_math("f32")
    g = la.glm_predictive_graph(x, quantiles=LEVELS, sigma=0.5, prior_precision=TAU)
    r = g.replay()
    e = la.glm_predictive(x, quantiles=LEVELS, sigma=0.5, prior_precision=TAU)
    assert _same(list(r), list(e)) and tuple(r.quantiles.shape) == (len(LEVELS), 5, 1)
    np.testing.assert_allclose(_np(r.predictive_variance), _np(r.variance) + 0.25, rtol=1e-6)
    z = G.normal_z(LEVELS)[1:-1]
    np.testing.assert_allclose(_np(r.quantiles[1:-1]), _np(r.mean)[None] + z[:, None, None] * np.sqrt(_np(r.variance))[None], rtol=1e-6)


def test_refusals_on_the_device(dev):
    bnn_hip.set_math("f32")
    mlp, la, x, _ = _fitted(dev, CASES[0])
    with pytest.raises(BnnHipError, match="link must be one of"):
        la.glm_predictive(x, link="logit")
    with pytest.raises(BnnHipError, match="samples >= 1"):
        la.glm_predictive(x, 0, link="mc")
    with pytest.raises(BnnHipError, match="regression summary"):
        la.glm_predictive(x, quantiles=[0.5])
    wide = _mlp(dev, "classification", 8, 8, 17)
    with pytest.raises(BnnHipError, match="at most 16 outputs"):
        wide.laplace().glm_moments(torch.zeros((2, 1, 1, 8), device=dev))
    bnn_hip.set_math("bf16")
    with pytest.raises(BnnHipError, match="math mode changed"):
        la.glm_moments(x, prior_precision=TAU)


# ------------------------------------------------------------------------------------------------------------ 7. non-finite input
def test_a_nan_curvature_entry_reaches_only_the_rows_it_belongs_to(dev):
    """NaN in F_b[o] of the second hidden layer: the rows whose unit o is active get NaN outputs, every other row stays finite."""
    case = CASES[0]
    mode, inp, hid, C, B, _ = case
    mlp, la, x, _ = _fitted(dev, case)
    bnn_hip.set_math("f32")
    ws = _weights(mlp)
    h = _np(x).reshape(B, -1)
    h = np.maximum(h @ ws[0][0].T + ws[0][1], 0.0)
    pre = h @ ws[1][0].T + ws[1][1]
    mixed = [(np.abs(pre[:, o]).min(), o) for o in range(hid) if 0 < (pre[:, o] > 0).sum() < B]
    margin, o = max(mixed)
    assert margin > 1e-4
    hit = pre[:, o] > 0
    saved = la.curv[3][o].clone()
    try:
        la.curv[3][o] = float("nan")
        p = la.glm_predictive(x, prior_precision=TAU)
        mean, cov = la.glm_moments(x, prior_precision=TAU)
        draws = la.glm_sample(x, 8, prior_precision=TAU, sample_offset=0).permute(1, 0, 2)
        torch.cuda.synchronize()
    finally:
        la.curv[3][o] = saved
    hit_t = torch.from_numpy(hit).to(dev)
    for t in (p.probs, p.predictive_entropy, cov, draws):
        flat = t.reshape(B, -1)
        assert bool(torch.isnan(flat[hit_t]).all()) and bool(torch.isfinite(flat[~hit_t]).all())
    assert bool(torch.isfinite(mean).all())
