"""SVGD / kde-WGD on the device (bnn_svgd_dist -> bnn_svgd_coef -> bnn_svgd_direction inside ensemble.EnsembleTrainStep,
bnn_hip.svgd; include/bnn_hip.h F23): each launch against fp64 with the bound the header states, the whole step graph against
eager, M = 1 against the plain step, one step end to end against torch autograd in fp64 through tests/svgd_ref.py, the sign of
the repulsion, the bank's consumers and the refusals.

Shapes are tests/test_gpu_ensemble.py's: 37-70-65-10 at batch 70 (stride 8256), 1-40-40-1 at batch 5 (stride 1920: a multiple
of 64 only) and 64-64-64-64 at batch 64 (stride 12480); at these sizes a chunk is one 64-column tile, so every case reduces
over many chunks (129, 30, 195).  M in {1, 2, 3, 9, 33, 64}:
fewer members than a 4 x 4 pair block, not a multiple of 4 or 16, more than 512 pairs (33, 64: the other reduction path of
bnn_svgd_coef) and the limit, 64 on the small regression net only."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import bnn_hip
import svgd_ref as R
from bnn_hip import _lib as L
from bnn_hip import ops
from bnn_hip.epoch import DeviceDataset, DeviceLoader, EpochRunner
from bnn_hip.ops import BnnHipError
from bnn_hip.optim import FusedAdam, FusedSGD
from bnn_hip.runtime import state
from test_gpu_ensemble import SEED, SHAPES, _batch, _ens, _net, _padding_mask

MEMBERS = {"c37": (1, 2, 3, 9, 33), "r1": (1, 2, 3, 9, 33, 64), "c64": (1, 2, 3, 9, 33)}
U24 = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore():
    yield
    bnn_hip.set_math("bf16")
    bnn_hip.manual_seed(2026)
    bnn_hip.shard_samples(False)


def _members(dev, shape, M, kind):
    """An M-member ensemble of SHAPES[shape] whose bank holds `kind` members: "seeded" (independent initialisations), "near"
    (theta_0 + 1e-4 noise with |theta_0| ~ 1: where the Gram identity loses every digit), "dup" (seeded, member 1 := member 0),
    "equal" (all members equal)."""
    net, ens = _ens(dev, shape, False, M)
    buf, pad = ens.bank.buffer, _padding_mask(ens.bank)
    g = torch.Generator().manual_seed(1000 + M)
    if kind == "near":
        base = torch.randn(buf.shape[1], generator=g)
        buf.copy_((base + 1e-4 * torch.randn(buf.shape, generator=g)).to(dev))
        buf[:, pad] = 0
    elif kind == "dup" and M > 1:
        buf[1].copy_(buf[0])
    elif kind == "equal":
        buf.copy_(buf[0].clone().expand_as(buf))
    return net, ens


def _gradients(dev, ens, seed=5):
    """A bucket of random gradients in the bank's layout, the padding zero."""
    b = torch.randn(ens.bank.buffer.shape, generator=torch.Generator().manual_seed(seed)).to(dev)
    b[:, _padding_mask(ens.bank)] = 0
    return b


# ------------------------------------------------------------------------------------------------ 1. distances, the record
@pytest.mark.parametrize("kind", ["seeded", "near", "dup"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_distances_and_median_against_fp64(dev, shape, kind):
    """D2 of the record against fp64 numpy on the bank read back: every entry within (L + 4) 2^-24 relative (a sum of
    non-negative terms: L = BNN_SVGD_CHAIN additions, 2 for the rounded difference squared, 2 to spare), exactly symmetric,
    the diagonal and a duplicate pair exactly 0; the median bit-equal to np.median of the device's own D2 (M^2 odd and even);
    h and r by their definitions from it."""
    assert L.SVGD_CHAIN == R.CHAIN == 129
    for M in MEMBERS[shape]:
        net, ens = _members(dev, shape, M, kind)
        tr = ens.svgd(dataset_size=700, batch_size=70)
        tr.enqueue(ens.bank, _gradients(dev, ens))
        rec = tr.read()
        want = R.dist2(ens.bank.buffer.cpu().numpy())
        assert rec.D2.shape == (M, M) and rec.D2.dtype == np.float64
        assert np.array_equal(rec.D2, rec.D2.T) and not rec.D2.diagonal().any(), (M, kind)
        err = np.abs(rec.D2 - want)
        worst = (err / np.where(want > 0, want, 1.0)).max()
        print(f"{shape} {kind} M={M}: worst relative D2 error {worst:.3e} (bound {(R.CHAIN + 4) * U24:.3e})")
        assert (err <= (R.CHAIN + 4) * U24 * want).all(), (M, kind, worst)
        if kind == "dup" and M > 1:
            assert rec.D2[0, 1] == 0.0 and rec.D2[1, 0] == 0.0
        if M > 2 and kind != "dup":
            assert (rec.D2[~np.eye(M, dtype=bool)] > 0).all()
        assert rec.median == np.median(rec.D2), (M, kind, rec.median, np.median(rec.D2))
        med, h = R.bandwidth(rec.D2)
        assert rec.h > 0 and abs(rec.h - h) <= 1e-15 * h, (M, kind, rec.h, h)
        if M == 1 or (kind == "dup" and M == 2):
            assert rec.median == 0.0 and rec.h == 1.0
        np.testing.assert_allclose(rec.r, R.kernel(rec.D2, rec.h)[1], rtol=1e-12)


# ------------------------------------------------------------------------------------------------ 2. the coefficients
@pytest.mark.parametrize("bandwidth", [None, 50.0], ids=["median", "fixed"])
@pytest.mark.parametrize("method", R.METHODS)
def test_coefficients_against_the_restatement_on_the_devices_distances(dev, method, bandwidth):
    """[A | B] against svgd_ref on the device's own fp64 D2: |err| <= 2^-22 of the largest term that enters the entry (one
    fp32 rounding, 2^-24, and the fp64 exp's and the expression's slack under it).  Seeded and near-collapsed members, M = 1
    and all-equal members (both h = 1 with the median rule).  The fixed bandwidth is of the order of the seeded members' D2, so
    every entry stays in fp32's normal range, where one rounding is 2^-24 relative (a kernel value under 2^-126 would carry
    fp32's absolute floor instead, which this bound does not describe)."""
    cases = [("r1", M, "seeded") for M in MEMBERS["r1"]] + [("c37", 9, "near"), ("c37", 1, "seeded"), ("c37", 3, "equal"), ("c64", 33, "near")]
    for shape, M, kind in cases:
        net, ens = _members(dev, shape, M, kind)
        kw = dict(dataset_size=6000, batch_size=70, prior_precision=0.8, temperature=0.5)
        tr = ens.svgd(method=method, bandwidth=bandwidth, **kw)
        s, tau = R.energy_scales(**kw)
        assert tr.grad_scale == s and tr.tau == tau
        tr.enqueue(ens.bank, _gradients(dev, ens))
        rec = tr.read()
        coef = tr.coef.cpu().numpy().astype(np.float64)
        assert coef.shape == (M, 2 * M)
        A, B, med, h, r = R.coefficients(rec.D2, s, tau, method, bandwidth)
        tA, tB = R.terms(rec.D2, s, tau, method, bandwidth)
        assert rec.median == med and abs(rec.h - h) <= 1e-15 * h
        if bandwidth is not None:
            assert rec.h == bandwidth
        elif M == 1 or kind == "equal":
            assert rec.h == 1.0
        eA, eB = np.abs(coef[:, :M] - A), np.abs(coef[:, M:] - B)
        assert np.isfinite(coef).all() and (np.abs(A[A != 0]) > 2.0 ** -126).all() and (np.abs(B[B != 0]) > 2.0 ** -126).all()
        assert (eA <= 2.0 ** -22 * tA).all(), (shape, M, kind, (eA / np.maximum(tA, 1e-300)).max())
        assert (eB <= 2.0 ** -22 * tB).all(), (shape, M, kind, (eB / np.maximum(tB, 1e-300)).max())
        if M == 1:
            assert coef[0, 0] == np.float32(s) and coef[0, 1] == np.float32(tau)


# ------------------------------------------------------------------------------------------------ 3. the direction
def _check_direction(dev, coef, bank0, g0, got, M, pad, what):
    C = coef.double()
    V = torch.cat([g0, bank0]).double()
    want = C @ V
    bound = (2 * M + 2) * U24 * (C.abs() @ V.abs())
    err = (got.double() - want).abs()
    assert bool((err <= bound).all()), (what, (err - bound).max().item())
    assert not got[:, pad].any(), what
    return (err / bound.clamp_min(1e-300)).max().item()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_direction_against_the_fp64_product_of_the_devices_coefficients(dev, shape):
    """bucket <- [A | B] . [bucket ; bank] elementwise against fp64 with the dot-product bound of one fp32 chain of 2 M terms,
    (2 M + 2) 2^-24 sum_k |c_k| |v_k|; padding columns exactly zero, the bank untouched bit for bit, two runs equal bits --
    with the coefficients of a whole enqueue (both methods) and with a dense random matrix in their place."""
    for M in MEMBERS[shape]:
        net, ens = _members(dev, shape, M, "seeded")
        pad = _padding_mask(ens.bank)
        bank0 = ens.bank.buffer.clone()
        g0 = _gradients(dev, ens)
        for method in R.METHODS:
            tr = ens.svgd(dataset_size=700, batch_size=70, method=method)
            runs = []
            for _ in range(2):
                bucket = g0.clone()
                tr.enqueue(ens.bank, bucket)
                runs.append(bucket)
            assert torch.equal(runs[0], runs[1]) and torch.equal(ens.bank.buffer, bank0), (M, method)
            assert not torch.equal(runs[0], g0)
            worst = _check_direction(dev, tr.coef, bank0, g0, runs[0], M, pad, (shape, M, method))
            print(f"{shape} M={M} {method}: worst error / bound {worst:.3f}")
        coef = torch.randn((M, 2 * M), generator=torch.Generator().manual_seed(M)).to(dev)
        bucket = g0.clone()
        ops.svgd_direction(coef, ens.bank.buffer, bucket, members=M)
        _check_direction(dev, coef, bank0, g0, bucket, M, pad, (shape, M, "random"))
        assert torch.equal(ens.bank.buffer, bank0)


# ------------------------------------------------------------------------------------------------ 4. the whole step
def _opt(kind, params, lr=None, wd=0.0):
    if kind == "sgd":
        return FusedSGD(params, lr=lr or 1e-3, weight_decay=wd, capturable=True)
    return FusedAdam(params, lr=lr or 1e-3, capturable=True)


def _train(dev, shape, dropout, M, kind, steps, capture, transform, counter=300, **tkw):
    _, _, B = SHAPES[shape]
    bnn_hip.set_math("f32")
    bnn_hip.manual_seed(SEED, counter)
    net, ens = _ens(dev, shape, dropout, M)
    opt = _opt(kind, ens.parameters())
    tr = ens.svgd(**tkw) if transform else None
    batches = [_batch(dev, net, B, seed=10 + t) for t in range(steps)]
    step = ens.graphed_train_step(opt, *batches[0], capture=capture, transform=tr)
    snaps = []
    for t in range(steps):
        loss = step.step(*batches[t]).clone()
        st = {k: v.clone() for k, v in opt.state[ens._param].items() if torch.is_tensor(v)}
        snaps.append((ens.bank.buffer.clone(), loss, st, None if tr is None else tr.record.clone()))
    return ens, step, snaps


@pytest.mark.parametrize("method", R.METHODS)
@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_graph_replays_match_eager_launches_bitwise_with_a_transform(dev, kind, method):
    M, steps, base = 3, 3, 300
    tkw = dict(dataset_size=700, batch_size=70, prior_precision=0.5, method=method)
    g = _train(dev, "c37", True, M, kind, steps, True, True, counter=base, **tkw)
    assert state.counter == base + M * steps and int(g[1].counter.item()) == M * steps     # M sample indices per step, as before
    e = _train(dev, "c37", True, M, kind, steps, False, True, counter=base, **tkw)
    plain = _train(dev, "c37", True, M, kind, steps, True, False, counter=base)
    assert g[1].graph is not None and e[1].graph is None
    assert g[1].launches == 11 and e[1].launches == 11 and plain[1].launches == 8
    for t, ((gb, gl, gs, gr), (eb, el, es, er)) in enumerate(zip(g[2], e[2])):
        assert torch.equal(gb, eb) and torch.equal(gl, el) and torch.equal(gr, er), t
        assert gs.keys() == es.keys() and all(torch.equal(gs[k], es[k]) for k in gs), t
        assert (gb[:, _padding_mask(g[0].bank)] == 0).all()
    assert torch.equal(g[2][0][1], plain[2][0][1])                       # the first step's losses are the untransformed forward's
    assert not torch.equal(g[2][-1][0], plain[2][-1][0])                 # the members are coupled


# ------------------------------------------------------------------------------------------------ 5. M = 1 is the plain step
@pytest.mark.parametrize("method", R.METHODS)
@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_one_member_is_the_plain_step_bitwise(dev, kind, method):
    """dataset_size == batch_size, temperature 1, prior_precision 0: A = [1], B = [0] exactly and the direction is g's bits."""
    tkw = dict(dataset_size=70, batch_size=70, prior_precision=0.0, temperature=1.0, method=method)
    a = _train(dev, "c37", True, 1, kind, 3, True, True, **tkw)
    b = _train(dev, "c37", True, 1, kind, 3, True, False)
    assert a[1].transform.coef.cpu().tolist() == [[1.0, 0.0]]
    assert a[1].launches == 11 and b[1].launches == 8
    for t, ((ab, al, ast, _), (bb, bl, bst, _)) in enumerate(zip(a[2], b[2])):
        assert torch.equal(ab, bb) and torch.equal(al, bl), t
        assert all(torch.equal(ast[k], bst[k]) for k in ast), t


# ------------------------------------------------------------------------------------------------ 6. end to end against fp64
@pytest.mark.parametrize("method", R.METHODS)
def test_one_sgd_step_end_to_end_against_fp64(dev, method):
    """One FusedSGD step (weight_decay 0) at 37-70-65-10, M = 9, f32 math, no dropout, against theta - lr d with d = svgd_ref's
    direction on fp64 autograd gradients of the sum loss.  The tolerance per element theta'_i[p], composed from what is already
    held elsewhere:
      * the gradients: tests/test_gpu_ensemble.py holds each kernel gradient tensor to 1e-5 of the reference tensor's largest
        magnitude Gmax_jt; through A that is sum_j |A_ij| 1e-5 Gmax_jt;
      * D2 (test 1): eps = (L + 4) 2^-24 relative per entry, hence for the median and h.  u e^-u <= 1 / e gives
        |delta k_ij| <= 2 eps / e < eps absolutely, |delta r_i| < M eps, and 2 / h moves by eps relative.  With c = 2 / h:
        svgd |delta A_ij| <= s eps / M, |delta B_ij| <= eps (tau' / M + 2 c);  wgd delta A = 0, |delta B_ij| <= c eps (M + 1)
        (r_i >= 1, k_ij / r_i <= 1);
      * the coefficients' rounding (test 2): 2^-22 of the largest term of the entry;
      * the product (test 3): (2 M + 2) 2^-24 sum_k |c_ik| |v_kp|;
      * the update fma(-lr, d, theta) and lr's own rounding: 2^-23 (|theta'| + lr |d|).
    Nothing here is fitted to the output; the figures observed are printed."""
    shape, M, lr = "c37", 9, 1e-3
    widths, mode, B = SHAPES[shape]
    bnn_hip.set_math("f32")
    bnn_hip.manual_seed(SEED, 77)
    net, ens = _ens(dev, shape, False, M)
    bank = ens.bank
    kw = dict(dataset_size=700, batch_size=70, prior_precision=0.5)
    s, tau = R.energy_scales(**kw)
    tr = ens.svgd(method=method, **kw)
    opt = FusedSGD(ens.parameters(), lr=lr, weight_decay=0.0, capturable=True)
    x, y = _batch(dev, net, B)
    start = bank.buffer.clone()
    step = ens.graphed_train_step(opt, x, y, transform=tr)
    step.step(x, y)
    theta = start.double()
    g64 = torch.zeros_like(theta)
    gmax = torch.zeros_like(theta)                                       # Gmax_jt spread over tensor t's columns
    for j in range(M):
        params = [theta[j, o:o + n].view(sh).clone().requires_grad_() for o, n, sh in zip(bank.offsets, bank.numels, bank.shapes)]
        h = x.reshape(B, -1).double()
        for l, d in enumerate(bank.layers):
            h = h @ params[2 * l].T + params[2 * l + 1]
            if d.relu:
                h = torch.relu(h)
        F.cross_entropy(h, y, reduction="sum").backward()
        for p, o, n in zip(params, bank.offsets, bank.numels):
            g64[j, o:o + n] = p.grad.reshape(-1)
            gmax[j, o:o + n] = p.grad.abs().max()
    th, g = theta.cpu().numpy(), g64.cpu().numpy()
    D2 = R.dist2(th)
    A, Bm, med, h, r = R.coefficients(D2, s, tau, method)
    tA, tB = R.terms(D2, s, tau, method)
    d = A @ g + Bm @ th
    want = th - lr * d
    eps, c = (R.CHAIN + 4) * U24, 2.0 / h
    if method == "svgd":
        dA, dB = np.full((M, M), s * eps / M), np.full((M, M), eps * (tau / M + 2 * c))
    else:
        dA, dB = np.zeros((M, M)), np.full((M, M), c * eps * (M + 1))
    dA, dB = dA + 2.0 ** -22 * tA, dB + 2.0 ** -22 * tB
    ag, ath = np.abs(g), np.abs(th)
    bound = lr * (np.abs(A) @ (1e-5 * gmax.cpu().numpy()) + dA @ ag + dB @ ath + (2 * M + 2) * U24 * (np.abs(A) @ ag + np.abs(Bm) @ ath)) \
        + 2.0 ** -23 * (np.abs(want) + lr * np.abs(d))
    got = bank.buffer.double().cpu().numpy()
    err = np.abs(got - want)
    pad = _padding_mask(bank).cpu().numpy()
    print(f"{method}: worst error / bound {(err[:, ~pad] / bound[:, ~pad]).max():.3f}; worst error {err.max():.3e}; "
          f"|lr d| max {np.abs(lr * d).max():.3e}")
    assert (err <= bound).all(), (err - bound).max()
    assert not got[:, pad].any() and np.abs(lr * d).max() > 100 * err.max()   # the step itself is far above its error


# ------------------------------------------------------------------------------------------------ 7. it repels
def test_near_collapsed_members_are_pushed_apart(dev):
    """Nine members = one network + 1e-3 noise, 20 steps on a fixed minibatch, the same energy in both runs (prior precision 1:
    in the transform, or as the plain optimiser's weight decay).  The smallest off-diagonal D2 grows with method="svgd" and
    does not grow without the transform: a sign check, larger against smaller only."""
    shape, M = "c37", 9
    _, _, B = SHAPES[shape]

    def run(transform):
        bnn_hip.set_math("f32")
        bnn_hip.manual_seed(SEED, 5)
        net, ens = _ens(dev, shape, False, M)
        buf, pad = ens.bank.buffer, _padding_mask(ens.bank)
        noise = torch.randn(buf.shape, generator=torch.Generator().manual_seed(3)).to(dev)
        buf.copy_(buf[0].clone().expand_as(buf) + 1e-3 * noise)
        buf[:, pad] = 0
        kw = dict(dataset_size=B, batch_size=B, prior_precision=1.0)
        probe = ens.svgd(**kw)                                           # measures D2 of the bank as it stands
        tr = ens.svgd(method="svgd", **kw) if transform else None
        opt = FusedSGD(ens.parameters(), lr=1e-3, weight_decay=0.0 if transform else 1.0, capturable=True)
        x, y = _batch(dev, net, B)
        step = ens.graphed_train_step(opt, x, y, transform=tr)

        def smallest():
            probe.enqueue(ens.bank, torch.zeros_like(buf))
            D2 = probe.read().D2
            return D2[~np.eye(M, dtype=bool)].min()

        before = smallest()
        for _ in range(20):
            step.step(x, y)
        if transform:                                                    # the step's own record: the state before its last update
            D2 = tr.read().D2
            assert D2[~np.eye(M, dtype=bool)].min() > before
        return before, smallest()

    b0, a0 = run(False)
    b1, a1 = run(True)
    print(f"smallest off-diagonal D2: plain {b0:.4e} -> {a0:.4e}; svgd {b1:.4e} -> {a1:.4e}")
    assert b0 == b1 and a1 > b1 and a0 <= b0


# ------------------------------------------------------------------------------------------------ 8. the consumers
def test_the_bank_feeds_its_consumers_and_an_epoch_runs(dev):
    widths, mode, B = SHAPES["c37"]
    M, nb = 3, 4
    bnn_hip.set_math("f32")
    bnn_hip.manual_seed(SEED, 10)
    net, ens = _ens(dev, "c37", True, M)
    xe, ye = _batch(dev, net, 33, seed=2)
    graph = ens.bank.predictive_graph(xe)                                 # captured before training
    before = graph.replay().probs.clone()
    g = torch.Generator().manual_seed(8)
    data_x = torch.rand((nb * B, 1, 1, widths[0]), generator=g)
    data_y = torch.randint(0, widths[-1], (nb * B,), generator=g)
    loader = DeviceLoader(DeviceDataset(data_x, data_y, device=dev), B, shuffle=True, seed=77)
    opt = FusedAdam(ens.parameters(), lr=1e-2, capturable=True)
    tr = ens.svgd(dataset_size=nb * B, batch_size=B, method="wgd")
    step = ens.graphed_train_step(opt, *loader.example(), transform=tr)
    start = ens.bank.buffer.clone()
    hist = EpochRunner(step, loader).run_epoch()
    assert hist.shape == (nb, M) and bool(torch.isfinite(hist).all()) and state.counter == 10 + M * nb
    assert not torch.equal(ens.bank.buffer, start)
    pred = ens.bank.predictive(xe)
    assert pred.probs.shape == (33, widths[-1]) and torch.allclose(pred.probs.sum(1), torch.ones(33, device=dev), atol=1e-5)
    after = graph.replay().probs
    assert torch.equal(after, pred.probs) and not torch.equal(after, before)     # the old graph sees the trained weights
    assert np.isfinite(ens.bank.score(xe, ye).read().lpd)
    rec = tr.read()
    assert rec.D2.shape == (M, M) and rec.h > 0 and (rec.r >= 1).all() and (rec.r <= M).all()


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_every_refusal_has_its_sentence(dev):
    from bnn_hip.svgd import SteinTransform
    bnn_hip.set_math("f32")
    net, ens = _ens(dev, "r1", False, 3)
    kw = dict(dataset_size=100, batch_size=5)
    with pytest.raises(BnnHipError, match="at most 64 members, got 65"):
        SteinTransform(net.ensemble(65), **kw)
    with pytest.raises(BnnHipError, match="method must be one of"):
        ens.svgd(method="stein", **kw)
    with pytest.raises(BnnHipError, match="prior_precision must be >= 0"):
        ens.svgd(prior_precision=-0.1, **kw)
    for t in (0.0, -1.0):
        with pytest.raises(BnnHipError, match="temperature must be > 0"):
            ens.svgd(temperature=t, **kw)
    for h in (0.0, -1.0):
        with pytest.raises(BnnHipError, match="bandwidth must be > 0"):
            ens.svgd(bandwidth=h, **kw)
    tr = ens.svgd(**kw)
    bucket = torch.zeros_like(ens.bank.buffer)
    with pytest.raises(BnnHipError, match="ROCm device only"):            # CPU tensors: no fallback
        tr.enqueue(ens.bank.buffer.cpu(), bucket.cpu())
    with pytest.raises(BnnHipError, match="the bank holds 2 members, 3 are needed"):
        tr.enqueue(ens.bank.buffer[:2], bucket)
    with pytest.raises(BnnHipError, match="in the bank's layout"):
        tr.enqueue(ens.bank, bucket[:2])
    x, y = _batch(dev, net, 5)
    other = net.ensemble(3, seeds=[1, 2, 3])
    with pytest.raises(BnnHipError, match="the transform must be built on this ensemble"):
        ens.graphed_train_step(FusedSGD(ens.parameters(), lr=1e-2, capturable=True), x, y, transform=other.svgd(**kw))
    empty = net.ensemble(3)                                               # fewer members in the bank than the ensemble has
    empty.bank.push(net)
    with pytest.raises(BnnHipError, match="holds 1 of 3 members"):
        empty.graphed_train_step(FusedSGD(empty.parameters(), lr=1e-2, capturable=True), x, y, transform=empty.svgd(**kw))
    with pytest.raises(BnnHipError, match="stride a multiple of 64"):
        ops.svgd_dist(torch.zeros((3, 100), device=dev), torch.zeros(3, device=dev), members=3)
