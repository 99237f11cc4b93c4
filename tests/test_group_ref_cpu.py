"""The float64 reference of the grouped bandit kernels (tests/group_ref.py) checked on the CPU, and proof that the bounds the
GPU tests derive from it (tests/test_gpu_group_steps.py) have teeth: the reference against itself (autograd against the header's
closed form, its Adam against torch.optim.Adam), every listed mistake planted in the float64 side and seen by the bound at the
very cases and seeds the GPU tests use, and every ReLU gate of those cases far enough from zero that fp32 and float64 agree on it."""
import functools

import numpy as np
import pytest
import torch

import group_ref as R

STEP_IDS = [c.id for c in R.STEP_CASES]
FWD_IDS = [c.id for c in R.FWD_CASES]
assert len(set(STEP_IDS)) == len(STEP_IDS) and len(set(FWD_IDS)) == len(FWD_IDS)


@functools.lru_cache(maxsize=None)
def _step(case):
    inp = R.inputs(case)
    ref = R.step64(case, inp)
    got = R.step32(case, inp)
    return inp, ref, got, R.deviations(got, ref)


# ---------------------------------------------------------------------------------------------------- the reference, itself
@pytest.mark.parametrize("case", [c for c in R.STEP_CASES if c.kind == "f7"], ids=lambda c: c.id)
def test_f7_autograd_equals_the_headers_closed_form(case):
    """g_mu = sum_s t_s, g_rho = (sum_s t_s eps_s - beta / sigma) sigmoid(rho), t_s = (d nll_s / dw - beta d log_p / dw) / S, in
    float64 against autograd through the loss as written, to 1e-12 of each tensor's largest gradient; loss_info likewise."""
    inp = R.inputs(case)
    eps = R._eps_lists(case, R.oracle_eps(case), case.counter)
    ps = [p.astype(R.F64) for p in inp["params"]]
    beta = float(R.F32(case.kl[0]))
    auto, info = R._gradients64(case, [torch.from_numpy(p) for p in ps], inp["slab"][0], inp["targets"][0], beta, eps)
    hand, hinfo = R.gradients_closed(case, ps, inp["slab"][0], inp["targets"][0], beta, eps, R.F64)
    for a, h in zip(auto, hand):
        assert h.dtype == R.F64
        assert R.rel_dev(h, a.numpy()) <= 1e-12
    scale = beta * (info["abs_q"] + info["abs_p"]) + info["loss_info"][3]
    assert np.abs(hinfo["loss_info"] - info["loss_info"]).max() <= 1e-12 * scale
    assert R.rel_dev(hinfo["z"], info["z"]) <= 1e-12


@pytest.mark.parametrize("case", [c for c in R.STEP_CASES if c.kind == "f6"], ids=lambda c: c.id)
def test_f6_autograd_equals_the_closed_form(case):
    inp = R.inputs(case)
    ps = [p.astype(R.F64) for p in inp["params"]]
    auto, info = R._gradients64(case, [torch.from_numpy(p) for p in ps], inp["slab"][0], inp["targets"][0], 0.0, None)
    hand, hinfo = R.gradients_closed(case, ps, inp["slab"][0], inp["targets"][0], 0.0, None, R.F64)
    for a, h in zip(auto, hand):
        assert R.rel_dev(h, a.numpy()) <= 1e-12
    assert abs(hinfo["loss"] - info["loss"]) <= 1e-12 * info["loss"]


@pytest.mark.parametrize("betas,eps,wd", [((0.8, 0.95), 1e-6, 1e-2), ((0.9, 0.999), 1e-8, 0.0)])
def test_adam_equals_torch_optim_adam(betas, eps, wd):
    """Three steps from a loaded state (step 7, non-zero moments) in float64 against torch.optim.Adam itself."""
    rs = np.random.RandomState(3)
    p0, m0 = rs.standard_normal((5, 7)), 0.3 * rs.standard_normal((5, 7))
    v0 = rs.uniform(0.01, 0.2, (5, 7))
    q = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([q], lr=1e-3, betas=betas, eps=eps, weight_decay=wd)
    opt.state[q] = dict(step=torch.tensor(7.0), exp_avg=torch.from_numpy(m0.copy()), exp_avg_sq=torch.from_numpy(v0.copy()))
    p, m, v = p0, m0, v0
    for k in range(3):
        g = rs.standard_normal((5, 7))
        q.grad = torch.from_numpy(g.copy())
        opt.step()
        p, m, v = R.adam(p, m, v, g, 7 + k + 1, 1e-3, betas, eps, wd)
        assert R.rel_dev(p, q.detach().numpy()) <= 1e-14
        assert R.rel_dev(m, opt.state[q]["exp_avg"].numpy()) <= 1e-14
        assert R.rel_dev(v, opt.state[q]["exp_avg_sq"].numpy()) <= 1e-14
    assert float(opt.state[q]["step"]) == 10


# ---------------------------------------------------------------------------------------------------- the bound's measurement
@pytest.mark.parametrize("case", R.STEP_CASES, ids=lambda c: c.id)
def test_d_ref_is_rounding_and_the_bound_holds_it(case):
    """d_ref is the fp32 restatement's own distance from float64: far below the cap at every case (a restatement that is merely
    wrong would sit at the cap and make every bound 2e-4), and the state the launch loads is what the issue asks for."""
    inp, ref, got, dref = _step(case)
    bnds = R.bounds(case, dref)
    print(f"  {case.id}: " + "; ".join(f"{c} d_ref {dref[c]:.2e} bound {bnds[c]:.2e}" for c in R.CLASSES))
    for c in R.CLASSES:
        assert bnds[c] < R.CAP
    assert all(np.abs(m).min() > 0 for m in inp["exp_avg"]) and all(v.min() > 0 for v in inp["exp_avg_sq"])
    assert ref["step"] == case.step0 + case.nb == 7 + case.nb
    tol = R.loss_tolerance(case, inp, ref, bnds)
    if case.kind == "f6":
        assert abs(float(got["loss"]) - ref["loss"]) <= tol
    else:
        assert (np.abs(got["loss_info"].astype(R.F64) - ref["loss_info"]) <= tol).all(), (got["loss_info"], ref["loss_info"], tol)


# ---------------------------------------------------------------------------------------------------- teeth
TEETH = [(c, p) for c in R.STEP_CASES for p in R.PERTURBATIONS if c.applies(p)]      # (a mistake that changes nothing at a
# case -- no weight decay to drop, S = 1, one minibatch, F7's terms at F6 -- is not run there)


def test_every_mistake_is_planted_somewhere():
    for p in R.PERTURBATIONS:
        assert sum(1 for c, q in TEETH if q == p) >= 2, p
    for c in R.STEP_CASES:
        assert {"t_minus_one", "betas_swapped"} <= {q for d, q in TEETH if d == c}


@pytest.mark.parametrize("case,perturbation", TEETH, ids=[f"{c.id}-{p}" for c, p in TEETH])
def test_the_bound_sees_a_planted_mistake(case, perturbation):
    """The float64 side with one mistake planted: the fp32 restatement of the right step must then miss 4 x d_ref (the bound
    the GPU test gives the kernel) on at least one of the tensors the GPU test compares."""
    inp, ref, got, dref = _step(case)
    bnds = R.bounds(case, dref)
    wrong = R.step64(case, inp, perturb=perturbation)
    seen = []
    for c in ("params", "exp_avg", "exp_avg_sq"):
        for i, (a, b) in enumerate(zip(got[c], wrong[c])):
            if R.rel_dev(a, b) > bnds[c]:
                seen.append((c, i, R.rel_dev(a, b) / bnds[c]))
    print(f"  {case.id} {perturbation}: {len(seen)} of {3 * len(got['params'])} tensors miss; worst "
          f"{max((s[2] for s in seen), default=0):.1f} x the bound")
    assert seen, (case.id, perturbation)


# ---------------------------------------------------------------------------------------------------- ReLU gates
@pytest.mark.parametrize("case", R.STEP_CASES, ids=lambda c: c.id)
def test_step_gates_keep_their_margin(case):
    inp, ref, got, dref = _step(case)
    margin = R.gate_margin(ref)
    print(f"  {case.id}: smallest |pre-activation| {margin[0]:.2e}, {margin[1]:.2e} of the layers' scale; needs > "
          f"{100 * dref['outputs']:.2e}")
    assert R.gate_margin_ok(ref, dref["outputs"]), (margin, dref["outputs"])


@pytest.mark.parametrize("case", R.FWD_CASES, ids=lambda c: c.id)
def test_forward_gates_keep_their_margin(case):
    inp = R.inputs(case, train=False)
    ref = R.forward64(case, inp)
    dref = R.d_ref(case, inp, ref, train=False)
    margin = R.gate_margin(ref)
    print(f"  {case.id}: d_ref {dref['outputs']:.2e}; smallest |pre-activation| {margin[0]:.2e}, {margin[1]:.2e} of scale")
    assert R.bound(dref["outputs"], R.FLOOR_OPS[case.kind]["outputs"]) < R.CAP
    assert R.gate_margin_ok(ref, dref["outputs"]), (margin, dref["outputs"])
