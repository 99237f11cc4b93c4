"""The diagonal Laplace posterior on the device (bnn_laplace_seed / _layer / _evidence / _posterior, bnn_hip.laplace.DiagLaplace;
include/bnn_hip.h F17): every stage against its fp64 restatement (tests/laplace_ref.py) computed from the kernel's own inputs,
the accumulated curvature end to end against the per-row Jacobian reference, the accumulation semantics bit for bit, the
evidence and the chosen precision, the (mu, rho) written, and the resulting BayesianNetwork under the existing tools.

Shapes: every edge of a 64-tile and of a 32-wide k stage is crossed -- classification 70-65-3 with batch 33 then 1 (R = 99, 3),
regression 1-40-1 with batch 5, classification 119-100-10 with batch 64 (R = 640: ten row tiles of the input-gradient product)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bnn_hip
import laplace_ref as R
from bnn_hip import _lib as L
from bnn_hip import ops, posthoc
from bnn_hip.ops import BnnHipError

#        mode, input, hidden, classes, batches
CASES = [("classification", 70, 65, 3, (33, 1)),
         ("regression", 1, 40, 1, (5,)),
         ("classification", 119, 100, 10, (64,))]
IDS = ["70-65-3", "1-40-1", "119-100-10"]
SIGMA = 0.8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore():
    yield
    bnn_hip.set_math("bf16")
    bnn_hip.manual_seed(2026)


def _mlp(dev, mode, inp, hid, C, seed=0, dropout=False):
    import networks
    torch.manual_seed(seed)
    cls = networks.MLP_Dropout if dropout else networks.MLP
    return cls(dict(input_shape=inp, classes=C, batch_size=128, hidden_units=hid, mode=mode)).to(dev)


def _batch(dev, mlp, B, seed):
    g = torch.Generator().manual_seed(seed)
    if mlp.mode == "classification":
        x = torch.rand((B, 1, 1, mlp.input_shape), generator=g) * 2 - 0.5
        return x.to(dev), torch.randint(0, mlp.classes, (B,), generator=g).to(dev)
    return torch.randn((B, mlp.input_shape), generator=g).to(dev), torch.randn((B, mlp.classes), generator=g).to(dev)


def _weights(mlp):
    return [(m.weight.detach().double().cpu().numpy(), m.bias.detach().double().cpu().numpy()) for m in mlp.net if hasattr(m, "weight")]


def _np(t):
    return t.detach().double().cpu().numpy()


def _close(got, ref, tol, what=""):
    """test_gpu_dense_train's max-norm check: |got - ref|_max <= tol * |ref|_max."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    scale = np.abs(ref).max()
    err = np.abs(got - ref).max()
    print(f"{what}: err {err:.3e} scale {scale:.3e} rel {err / max(scale, 1e-300):.3e} (tol {tol:.1e})")
    assert err <= tol * max(scale, 1e-30), (what, err, scale)


def _bf16(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).to(torch.bfloat16).double().numpy()


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
    curv = [torch.zeros_like(t) for m in lins for t in (m.weight, m.bias)]
    record = torch.zeros(2, dtype=torch.float64, device=dev)
    rec_ref = np.zeros(2)
    for bi, B in enumerate(batches):
        x, y = _batch(dev, mlp, B, seed=10 + bi)
        xf = x.reshape(B, -1).contiguous()
        # the forward: exact fp32 here whatever the math mode, so that every later stage sees the same inputs
        acts, h = [], xf
        for i, m in enumerate(lins):
            h = ops.dense_fwd(h, m.weight.detach(), m.bias.detach(), n_samples=1, math_mode=L.MATH_F32, relu=i < 2, drop_p=0.0,
                              layer_id=i, seed=0, y_dtype=torch.float32)[0]
            acts.append(h)
        gy = ops.laplace_seed(acts[-1], y, mode, curvature=curvature, sigma=SIGMA, record=record)
        ref_gy, ref_ll = R.seed(_np(acts[-1]), y.cpu().numpy(), mode, curvature, SIGMA)
        assert gy.shape == ref_gy.shape == (ops.laplace_rows(B, C, curvature), C)
        _close(_np(gy), ref_gy, 1e-5, f"seed b{B}")
        rec_ref += (ref_ll, B)
        got_rec = record.cpu().numpy()
        assert got_rec[1] == rec_ref[1] and abs(got_rec[0] - rec_ref[0]) <= 1e-12 * abs(rec_ref[0]), (got_rec, rec_ref)
        g = gy
        for i in (2, 1, 0):
            xin = xf if i == 0 else acts[i - 1]
            w = lins[i].weight.detach()
            before = [_np(curv[2 * i]), _np(curv[2 * i + 1])]
            s_out = torch.full((B, w.shape[0]), float("nan"), device=dev)
            gx = torch.full((g.shape[0], w.shape[1]), float("nan"), device=dev) if i > 0 else None
            ops.laplace_layer(xin, g, w, f_w=curv[2 * i], f_b=curv[2 * i + 1], g_x=gx, y=acts[i] if i < 2 else None, gx_mask=i > 0,
                              s_out=s_out, math_mode=mm)
            S, dfw, dfb, _ = R.layer(_np(xin), _np(g), _np(acts[i]) if i < 2 else None, _np(w), want_gx=False)
            _close(_np(s_out), S, 1e-5, f"S{i} b{B}")
            # F_w and F_b from the kernel's own S and its own stored values: the two products of the layer launch
            S_k = _np(s_out)
            _close(_np(curv[2 * i]), before[0] + S_k.T @ _np(xin) ** 2, 1e-5, f"F_w{i} b{B}")
            _close(_np(curv[2 * i + 1]), before[1] + S_k.sum(0), 1e-5, f"F_b{i} b{B}")
            _close(_np(curv[2 * i]), before[0] + dfw, 1e-5, f"F_w{i} b{B} (restated S)")
            _close(_np(curv[2 * i + 1]), before[1] + dfb, 1e-5, f"F_b{i} b{B} (restated S)")
            if i > 0:
                gz = _np(g).reshape(-1, B, w.shape[0])
                if i < 2:
                    gz = np.where((_np(acts[i]) > 0)[None], gz, 0.0)
                gz = gz.reshape(g.shape[0], -1)
                ref_gx = (_bf16(gz) @ _bf16(_np(w))) if math_mode == "bf16" else gz @ _np(w)
                ref_gx = np.where(np.tile(_np(xin) > 0, (g.shape[0] // B, 1)), ref_gx, 0.0)
                _close(_np(gx), ref_gx, tol_gx, f"g_x{i} b{B}")
                g = gx
    assert all(bool(torch.isfinite(t).all()) and bool((t >= 0).all()) for t in curv)


# ------------------------------------------------------------------------------------------------------------ 2. end to end
def _two_batches(case):
    return case[4] if len(case[4]) == 2 else case[4] * 2


def _relu_margin(weights, xs):
    """(the smallest |pre-activation| of a hidden unit over the inputs in fp64, the largest error of the same pre-activations
    computed in fp32 by torch on the CPU)."""
    m, err = np.inf, 0.0
    for x in xs:
        h, h32 = x, torch.tensor(x, dtype=torch.float32)
        for w, b in weights[:-1]:
            z = h @ w.T + b
            z32 = h32 @ torch.tensor(w, dtype=torch.float32).T + torch.tensor(b, dtype=torch.float32)
            m, err = min(m, np.abs(z).min()), max(err, np.abs(z32.double().numpy() - z).max())
            h, h32 = np.maximum(z, 0.0), torch.relu(z32)
    return m, err


@pytest.mark.parametrize("curvature", ["ggn", "empirical"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_two_minibatches_against_the_jacobian_reference(dev, case, curvature):
    """Bound: 10 x the max-norm error (relative to each tensor's largest entry; the largest over the six tensors) of the same
    formula evaluated in plain fp32 by torch on the CPU against fp64, on the same inputs.  The factor covers another summation
    order on the device.  No hidden pre-activation may lie within 8 x the fp32 forward's own error of zero (asserted first):
    the comparison is of the arithmetic, not of which side of a ReLU tie a rounding lands on."""
    mode, inp, hid, C, _ = case
    bnn_hip.set_math("f32")
    mlp = _mlp(dev, mode, inp, hid, C, seed=1)
    la = bnn_hip.DiagLaplace(mlp, curvature=curvature, sigma=SIGMA)
    weights = _weights(mlp)
    xs, ys = [], []
    for bi, B in enumerate(_two_batches(case)):
        x, y = _batch(dev, mlp, B, seed=22 + bi)
        la.accumulate(x, y)
        xs.append(_np(x).reshape(B, -1))
        ys.append(y.cpu().numpy())
    margin, fwd_err = _relu_margin(weights, xs)
    assert margin > 8 * fwd_err, (margin, fwd_err)
    base, restated = R.fp32_chain_error(weights, xs, ys, mode, curvature, SIGMA)
    ref = sum(R.jacobian_curvature(weights, x, y, mode, curvature, SIGMA) for x, y in zip(xs, ys))
    flat = np.concatenate([r.reshape(-1) for r in restated])
    assert np.abs(flat - ref).max() <= 1e-11 * np.abs(ref).max()          # the two fp64 forms agree
    print(f"{IDS[CASES.index(case)]} {curvature}: fp32 base error {base:.3e}, bound {10 * base:.3e}")
    assert 0 < base < 1e-5
    at = 0
    for t, name in zip(la.curv, ("F_w0", "F_b0", "F_w1", "F_b1", "F_w2", "F_b2")):
        r = ref[at:at + t.numel()].reshape(tuple(t.shape))
        at += t.numel()
        _close(_np(t), r, 10 * base, name)
    assert la.n_rows == sum(_two_batches(case))


# ------------------------------------------------------------------------------------------------------------ 3. accumulation
def _bits(la):
    return [t.clone() for t in la.curv] + [la.record.clone()]


def _same(a, b):
    return all(torch.equal(s.view(torch.uint8), t.view(torch.uint8)) for s, t in zip(a, b))


def test_accumulation_is_deterministic_and_reset_zeroes(dev):
    bnn_hip.set_math("f32")
    mode, inp, hid, C, batches = CASES[0]
    mlp = _mlp(dev, mode, inp, hid, C)
    data = [_batch(dev, mlp, B, seed=30 + i) for i, B in enumerate(batches)]
    runs = []
    for _ in range(2):
        la = mlp.laplace()
        for x, y in data:
            la.accumulate(x, y)
        runs.append(_bits(la))
    assert _same(*runs) and any(bool((t != 0).any()) for t in runs[0])
    one = mlp.laplace()
    one.accumulate(*data[0])
    assert not _same(_bits(one), runs[0])                                  # the second minibatch did add something
    la.reset()
    assert all(bool((t == 0).all()) for t in _bits(la))
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
    eager, graphed = mlp.laplace(sigma=SIGMA), mlp.laplace(sigma=SIGMA)
    step = graphed.accumulate_graph(*data[0])
    assert all(bool((t == 0).all()) for t in _bits(graphed))               # building the step accumulates nothing
    for x, y in data:
        eager.accumulate(x, y)
        step.step(x, y)
    assert _same(_bits(eager), _bits(graphed)) and eager.n_rows == 5 * B
    assert graphed.accumulate_graph(*data[0])._chain is step._chain        # one capture per batch size


def test_fit_twice_gives_the_same_bits(dev):
    bnn_hip.set_math("f32")
    mode, inp, hid, C, batches = CASES[0]
    mlp = _mlp(dev, mode, inp, hid, C)
    loader = [_batch(dev, mlp, B, seed=50 + i) for i, B in enumerate((33, 33, 1))]
    la = mlp.laplace(curvature="empirical")
    first = _bits(la.fit(loader))
    assert la.n_rows == 67
    assert _same(first, _bits(la.fit(loader)))


# ------------------------------------------------------------------------------------------------------------ 4. evidence
@pytest.fixture(scope="module")
def fitted(dev):
    """One fitted 70-65-3 posterior shared by the read-only tests below."""
    bnn_hip.set_math("f32")
    mode, inp, hid, C, _ = CASES[0]
    mlp = _mlp(dev, mode, inp, hid, C, seed=2)
    data = [_batch(dev, mlp, 33, seed=60 + i) for i in range(4)]
    la = mlp.laplace().fit(data)
    bnn_hip.set_math("bf16")
    return mlp, la, data


def test_log_evidence_and_the_chosen_precision(dev, fitted):
    mlp, la, _ = fitted
    taus = np.logspace(-4, 4, 9)
    got = la.log_evidence(taus)
    assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == (9,)
    params, curvs = [_np(p) for p in la.params], [_np(f) for f in la.curv]
    rec = la.record.cpu().numpy()
    ref = R.evidence(params, curvs, taus, rec[0])
    w = np.concatenate([p.reshape(-1) for p in params])
    f = np.concatenate([c.reshape(-1) for c in curvs])
    eps = 2.0 ** -53
    for g, (t, r) in enumerate(zip(taus, ref)):
        # the fp64 sums' own bound: P terms, each within P eps of the running sum of magnitudes (the tree is tighter)
        mag = 0.5 * np.abs(np.log(f + t)).sum() + 0.5 * t * (w ** 2).sum() + abs(0.5 * w.size * math.log(t)) + abs(rec[0])
        assert abs(got[g].item() - r) <= 1e-12 * abs(r) + w.size * eps * mag, (g, got[g].item(), r)
    best, gap = R.best_precision(ref)
    assert gap > 1e-9                                                       # the index cannot hinge on the summation order
    again = la.fit_prior_precision(taus)
    assert torch.equal(again, got)
    assert int(la._best_index.item()) == best == int(np.argmax(ref))
    assert la.prior_precision == taus[best]
    assert abs(la._best[0].item() - ref[best]) <= 1e-12 * abs(ref[best]) + w.size * eps * mag
    full = la.fit_prior_precision()                                         # the default grid: 33 candidates in one pass
    assert tuple(full.shape) == (33,) and bool(torch.isfinite(full).all())
    assert la.prior_precision == np.logspace(-4, 4, 33)[int(torch.argmax(full).item())]
    with pytest.raises(BnnHipError):
        la.log_evidence(np.logspace(-4, 4, L.LAPLACE_MAX_PRECISIONS + 1))


# ------------------------------------------------------------------------------------------------------------ 5. posterior
def test_posterior_mu_and_rho(dev):
    """softplus(rho) in fp64 against (F + tau)^-1/2 to rtol 4e-6: storing rho in fp32 costs |rho| 2^-24 <= 1e-6 relative on
    sigma for sigma >= 1e-7 (sigma ~ e^rho at the small end, rho ~ sigma at the large end); x 4 for the kernel's log / expm1."""
    g = torch.Generator().manual_seed(7)
    n = 5000                                                                # two chunks of the first tensor
    w = [torch.randn(n, generator=g).to(dev), torch.randn((3, 7), generator=g).to(dev)]
    f0 = torch.cat([torch.zeros(8), torch.logspace(-12, 12, n - 8, dtype=torch.float64).float()])
    f = [f0.to(dev), (torch.rand((3, 7), generator=g) * 50).to(dev)]
    for tau in (1e-4, 1.0, 1e4, 1e12):
        mus = [torch.full_like(t, float("nan")) for t in w]
        rhos = [torch.full_like(t, float("nan")) for t in w]
        ops.laplace_posterior(w, f, mus, rhos, precision=tau)
        word = torch.tensor([tau], dtype=torch.float64, device=dev)
        mus2, rhos2 = [torch.empty_like(t) for t in w], [torch.empty_like(t) for t in w]
        ops.laplace_posterior(w, f, mus2, rhos2, precision_device=word)
        for wi, fi, mu, rho, mu2, rho2 in zip(w, f, mus, rhos, mus2, rhos2):
            assert torch.equal(mu.view(torch.int32), wi.view(torch.int32)) and torch.equal(mu2.view(torch.int32), wi.view(torch.int32))
            assert torch.equal(rho.view(torch.int32), rho2.view(torch.int32))          # the device word gives the same bits
            assert bool(torch.isfinite(rho).all())
            want = R.posterior_sigma(_np(fi), tau)
            got = R.softplus(_np(rho))
            rel = np.abs(got - want) / want
            print(f"tau {tau:g}: sigma in [{want.min():.3e}, {want.max():.3e}], max rel err {rel.max():.3e}")
            assert rel.max() <= 4e-6


# ------------------------------------------------------------------------------------------------------------ 6. a real network
def test_the_product_is_an_ordinary_bayesian_network(dev, fitted):
    import networks
    mlp, la, data = fitted
    bnn_hip.set_math("f32")
    la.fit_prior_precision()
    tau = la.prior_precision
    net = la.network()
    assert isinstance(net, networks.BayesianNetwork) and net.mixture_prior is False and net.local_reparam is False
    assert net.prior_init == [tau ** -0.5] and net.mode == mlp.mode
    assert (net.input_shape, net.hidden_units, net.classes, net.batch_size) == (mlp.input_shape, mlp.hidden_units, mlp.classes, mlp.batch_size)
    lins = [m for m in mlp.net if hasattr(m, "weight")]
    for lay, lin, fw, fb in zip((net.l1, net.l2, net.l3), lins, la.curv[0::2], la.curv[1::2]):
        assert torch.equal(lay.weight_mu.data, lin.weight.data) and torch.equal(lay.bias_mu.data, lin.bias.data)
        for rho, f_ in ((lay.weight_rho, fw), (lay.bias_rho, fb)):
            want = R.posterior_sigma(_np(f_), tau)
            assert (np.abs(R.softplus(_np(rho)) - want) / want).max() <= 4e-6
    x, y = data[0]
    net.eval()
    with torch.no_grad():
        out = net.forward(x, sample=False)
        _close(_np(out), _np(mlp(x)), 1e-5, "mean forward")
        fresh = networks.BayesianNetwork(dict(input_shape=mlp.input_shape, classes=mlp.classes, batch_size=mlp.batch_size,
                                              hidden_units=mlp.hidden_units, mode=mlp.mode, mu_init=[-0.2, 0.2], rho_init=[-5, -4],
                                              prior_init=net.prior_init, mixture_prior=False, local_reparam=False))
        fresh.load_state_dict(net.state_dict())
        fresh.to(dev).eval()
        assert torch.equal(fresh.forward(x, sample=False), out)
        preds, probs = net.predict_mc(x, 8)
        assert tuple(probs.shape) == (33, 3) and bool(torch.isfinite(probs).all()) and tuple(preds.shape) == (33,)
        sc = net.score(x, y, 8).read()
        assert sc.n == 33 and math.isfinite(sc.lpd) and math.isfinite(sc.nll) and math.isfinite(sc.brier)
        sweep = posthoc.PruneSweep(net)
        res = sweep.evaluate((x, y))
        assert bool(torch.isfinite(sweep.thresholds).all()) and np.isfinite(res.accuracy).all() and np.isfinite(res.nll).all()
    explicit = la.network(prior_precision=3.0)                              # a host value instead of the device word
    assert explicit.prior_init == [3.0 ** -0.5]
    want = R.posterior_sigma(_np(la.curv[0]), 3.0)
    assert (np.abs(R.softplus(_np(explicit.l1.weight_rho)) - want) / want).max() <= 4e-6


# ------------------------------------------------------------------------------------------------------------ 7. failure modes
@pytest.mark.parametrize("curvature", ["ggn", "empirical"])
def test_out_of_range_label_gives_nan_and_no_fault(dev, curvature):
    bnn_hip.set_math("f32")
    mode, inp, hid, C, _ = CASES[0]
    mlp = _mlp(dev, mode, inp, hid, C)
    x, y = _batch(dev, mlp, 5, seed=70)
    y = y.clone()
    y[2] = C                                                                # one past the last class
    y[4] = -1
    z = mlp(x).detach().contiguous()
    record = torch.zeros(2, dtype=torch.float64, device=dev)
    gy = ops.laplace_seed(z, y, mode, curvature=curvature, record=record).reshape(-1, 5, C)
    torch.cuda.synchronize()
    assert bool(torch.isnan(gy[:, [2, 4]]).all()) and bool(torch.isfinite(gy[:, [0, 1, 3]]).all())
    assert math.isnan(record[0].item()) and record[1].item() == 5
    la = mlp.laplace(curvature=curvature)
    la.accumulate(x, y)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).any()) for t in la.curv)


def test_dropout_on_is_refused_and_off_is_accepted(dev):
    bnn_hip.set_math("f32")
    mode, inp, hid, C, _ = CASES[0]
    drop = _mlp(dev, mode, inp, hid, C, dropout=True)
    with pytest.raises(BnnHipError, match="dropout is on"):
        drop.laplace()
    drop.eval()
    plain = _mlp(dev, mode, inp, hid, C)
    plain.load_state_dict({k.replace("net.3", "net.2").replace("net.6", "net.4"): v for k, v in drop.state_dict().items()})
    x, y = _batch(dev, drop, 33, seed=80)
    a, b = drop.laplace(), plain.laplace()
    a.accumulate(x, y)
    b.accumulate(x, y)
    assert _same(_bits(a), _bits(b))                                        # the same weights, the same curvature
