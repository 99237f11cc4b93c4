"""The layer backward kernels (bnn_bbb_linear_bwd: csrc/bbb_bwd.hip and the TRANS forms of csrc/bbb_linear.hip;
bnn_lr_linear_bwd: csrc/lr_bwd.hip) on an MI355X against the fp64 restatement tests/layer_bwd_ref.py: EVERY element of every
returned tensor under its own derived bound (the derivation is that module's docstring; tests/test_layer_bwd_cpu.py proves
the restatement against autograd, the bound wide enough for fp32 and tight enough for seeded wrong variants).  Every case
runs twice: with upstream KL gradients, and with g_log_prior = g_log_q = g_kl = None (the data term alone).

Nothing was tuned on the device's figures; measured afterwards (largest |got - ref| / bound over a tensor's elements):
                       g_w_mu  g_w_rho  g_b_mu  g_b_rho  g_x
  with upstream KL gradients
    BBB general        0.268   0.228    0.187   0.082    0.212
    BBB narrow output  0.102   0.102    0.024   0.023    0.070
    BBB full-width     0.237   0.178    0.137   0.078    0.001
    LR general         0.065   0.052    0.059   0.041    0.030
    LR narrow output   0.012   0.024    0.003   0.017    0.082
  the data term alone
    BBB general        0.086   0.316    0.059   0.232    0.212
    BBB narrow output  0.005   0.017    0.003   0.008    0.070
    BBB full-width     0.108   0.148    0.051   0.118    0.001
    LR general         0.063   0.196    0.048   0.155    0.030
    LR narrow output   0.010   0.036    0.003   0.008    0.082
g_x above leaves out the six bf16-math cases in which a re-created operand lies within its fp32 error of a bf16 rounding tie
(0.04 % .. 0.17 % of the operands): there the device took the other neighbour for some of them, which the bound allows for
exactly those operands, and the share is that allowance's: 0.996 (w-grid15of16), 0.967 (lr-72-bf16-wide), 0.375 (lr-72-bf16),
0.299 (lr-72-hfac-bf16), 0.023 (w-s5-gauss), 0.021 (w-b1).  ops.softplus: 14.953 u at its worst (rho = -12), E_T = 32.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import layer_bwd_ref as R
from bnn_hip import _lib as L
from bnn_hip import ops


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


def _up(a, dev):
    return None if a is None else (a if torch.is_tensor(a) else torch.from_numpy(a)).to(dev)


def _check(what, got, ref):
    sh = R.shares([g.cpu() for g in got[:5]], ref)
    print(f"{what:26s} share of the bound: " + "  ".join(f"{n} {s:.3f}" for n, s in zip(R.NAMES, sh))
          + f"  ties {ref.info['tie_share']:.4f}")
    assert max(sh) <= 1.0, (what, dict(zip(R.NAMES, sh)))


def test_softplus_error_constant(dev):
    """E_T: the one measured constant of the bound.  Largest relative error of ops.softplus against fp64 log1p(exp(rho)), in
    units of 2^-24, over 4096 evenly spaced rho in [-12, 2] and the fp32 neighbours of the cases' rho end points."""
    rho = R.softplus_probe_points()
    got = ops.softplus(torch.from_numpy(rho).to(dev)).cpu().numpy()
    measured = R.softplus_error_in_u(got, rho)
    print(f"softplus: largest relative error {measured:.3f} u (recorded {R.E_T_MEASURED}, E_T = {R.E_T})")
    assert measured <= R.E_T / 2


def _bbb_call(c, d, kl, dev):
    S = c["S"]
    pr = d["prior"]
    mem = c["eps"] == "memory"
    kw = dict(n_samples=S, prior=ops.PriorSpec(pr.mixture, pr.sigma_p, pr.pi, pr.sigma1, pr.sigma2),
              math_mode=L.MATH_BF16 if c["math"] == "bf16" else L.MATH_F32, relu=c["relu"],
              eps_mode=L.EPS_MEMORY if mem else L.EPS_PHILOX, seed=R.SEED, layer_id=R.LAYER_ID, sample_offset=R.SAMPLE_OFFSET,
              gx_relu_mask=c["mask"], want_gx16=c["gx16"])
    if mem:
        kw.update(eps_w=_up(d["eps_w"][:S], dev), eps_b=_up(d["eps_b"][:S], dev))
    if c["counter"]:
        kw["sample_counter"] = torch.tensor([c["counter"]], dtype=torch.int32, device=dev)
    if kl == "kl":
        kw.update(g_log_prior=_up(d["glp"], dev), g_log_q=_up(d["glq"], dev))
    gy = _up(d["gy"], dev)
    if c["wsrc"]:
        kw["w_sampled"] = _up(d["w_sampled"], dev)
    if c["wsrc"] == "wt":
        kw["w_sampled_t"] = kw["w_sampled"].transpose(1, 2).contiguous()
        if c["gy16"]:
            kw["gy16"] = gy.to(torch.bfloat16)
    return ops.bbb_linear_bwd(_up(d["x"], dev), gy, _up(d["y"], dev), _up(d["w_mu"], dev), _up(d["w_rho"], dev),
                              _up(d["b_mu"], dev), _up(d["b_rho"], dev), **kw)


@pytest.mark.parametrize("kl", R.KL_MODES)
@pytest.mark.parametrize("name", list(R.BBB_CASES))
def test_bbb_backward_within_the_fp64_bound(dev, name, kl):
    c, d = R.BBB_CASES[name], R.bbb_inputs(name)
    got = _bbb_call(c, d, kl, dev)
    _check(f"{name} {kl}", got, R.bbb_run(name, kl))
    if c["gx16"]:
        assert torch.equal(got[5], got[4].to(torch.bfloat16))      # the bf16 copy is bf16(g_x), bit for bit


@pytest.mark.parametrize("kl", R.KL_MODES)
def test_bbb_backward_full_width_within_the_fp64_bound(dev, kl):
    """(1, 16, 1200, 1200): the XCD work-item mapping over 722 blocks.  Epsilon from ops.philox_normal (bit-pinned to the
    CPU restatement by test_philox_matches_cpu_restatement; 1.4 M draws of it here would be seconds of numpy)."""
    c = R.BBB_FULL
    S, B, K, N = c["S"], c["B"], c["K"], c["N"]
    d, f = R._common(c, R._rs("full-width"), False)
    rs = R._rs("full-width-kl")
    d.update(glp=f(rs.uniform(-0.5, 0.5, S)), glq=f(rs.uniform(-0.5, 0.5, S)), w_sampled=None, prior=R.MIX)
    d["eps_w"] = ops.philox_normal(R.SEED, 4 * R.LAYER_ID + 0, d["sample0"], S, N, K, dev).cpu().numpy()
    d["eps_b"] = ops.philox_normal(R.SEED, 4 * R.LAYER_ID + 1, d["sample0"], S, 1, N, dev).cpu().numpy().reshape(S, N)
    got = _bbb_call(c, d, kl, dev)
    _check(f"full-width {kl}", got, R.bbb_run("full-width", kl, inputs=d))


@pytest.mark.parametrize("kl", R.KL_MODES)
@pytest.mark.parametrize("name", list(R.LR_CASES))
def test_lr_backward_within_the_fp64_bound(dev, name, kl):
    c, d = R.LR_CASES[name], R.lr_inputs(name)
    S = c["S"]
    mem = c["eps"] == "memory"
    factor = c["mode"] == "hfac"
    kw = dict(n_samples=S, sigma_p=d["sigma_p"], relu=c["relu"], eps_mode=L.EPS_MEMORY if mem else L.EPS_PHILOX, seed=R.SEED,
              layer_id=R.LAYER_ID, sample_offset=R.SAMPLE_OFFSET, gx_relu_mask=c["mask"],
              math_mode=L.MATH_BF16 if c["math"] == "bf16" else L.MATH_F32)
    if mem:
        kw.update(eps_act=_up(d["eps_act"][:S], dev), eps_b=_up(d["eps_b"][:S], dev))
    if c["counter"]:
        kw["sample_counter"] = torch.tensor([c["counter"]], dtype=torch.int32, device=dev)
    if kl == "kl":
        kw["g_kl"] = _up(d["gkl"], dev)
    if factor:
        kw["hfac"] = _up(d["hfac"], dev)
    got = ops.lr_linear_bwd(_up(d["x"], dev), _up(d["gy"], dev), _up(d["y"], dev), None if factor else _up(d["v"], dev),
                            _up(d["w_mu"], dev), _up(d["w_rho"], dev), _up(d["b_mu"], dev), _up(d["b_rho"], dev), **kw)
    _check(f"{name} {kl}", got, R.lr_run(name, kl))
