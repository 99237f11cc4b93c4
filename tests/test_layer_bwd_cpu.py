"""The fp64 restatement of the layer backward (tests/layer_bwd_ref.py) and its bound, proven without a GPU:
 1. the restatement equals torch autograd in fp64 on the forward formulas, elementwise to 1e-11 relative;
 2. the same formulas in fp32 (torch-CPU, plain order) lie inside the bound at every case of the GPU matrix
    (tests/test_gpu_layer_bwd.py; all but the full-width one), the largest share err / bound printed per case;
 3. seeded wrong variants of the restatement break the bound at every case they apply to."""
import math

import numpy as np
import pytest
import torch

import layer_bwd_ref as R

F64 = torch.float64
ALL = [("bbb", n) for n in R.BBB_CASES] + [("lr", n) for n in R.LR_CASES]


def _run(kind, name, kl, **kw):
    return (R.bbb_run if kind == "bbb" else R.lr_run)(name, kl, **kw)


# ------------------------------------------------------------------------------------------ 1. restatement == autograd
def _rel_equal(got, want, what):
    for n, a, b in zip(R.NAMES, got, want):
        assert torch.equal(a == 0, b == 0), (what, n)
        err = (a - b).abs()
        assert bool((err <= 1e-11 * b.abs()).all()), (what, n, float((err / b.abs().clamp_min(1e-300)).max()))


def _log_normal(w, mu, sigma):
    return -0.5 * math.log(2 * math.pi) - torch.log(sigma) - (w - mu) ** 2 / (2 * sigma ** 2)


def _log_prior(w, pr):
    if not pr.mixture:
        return _log_normal(w, 0.0, torch.tensor(pr.sigma_p, dtype=F64)).sum()
    l1 = math.log(pr.pi) + _log_normal(w, 0.0, torch.tensor(pr.sigma1, dtype=F64))
    l2 = math.log(1 - pr.pi) + _log_normal(w, 0.0, torch.tensor(pr.sigma2, dtype=F64))
    return torch.logsumexp(torch.stack([l1, l2]), 0).sum()


@pytest.mark.parametrize("kl", R.KL_MODES)
@pytest.mark.parametrize("name", ["w-vec-philox", "w-vec-mem", "w-n1-gauss", "w-s5", "w-novec-philox"])
def test_bbb_restatement_equals_autograd_in_fp64(name, kl):
    """y = relu(x W^T + b), log p and log q with w = mu + softplus(rho) * eps; y (the ReLU mask) is the fp64 forward's own
    output here, which has no exact zero: autograd's mask convention is not what is being tested."""
    c, d = R.BBB_CASES[name], R.bbb_inputs(name)
    S = c["S"]
    t = lambda a: torch.from_numpy(a).to(F64)
    x = t(d["x"]) if c["x3"] else t(d["x"]).unsqueeze(0).repeat(S, 1, 1)
    x = x.clone().requires_grad_(True)
    P = [t(d[k]).clone().requires_grad_(True) for k in ("w_mu", "w_rho", "b_mu", "b_rho")]
    eps_w, eps_b = t(d["eps_w"][:S]), t(d["eps_b"][:S])
    sw, sb = torch.log1p(torch.exp(P[1])), torch.log1p(torch.exp(P[3]))
    W, b = P[0] + sw * eps_w, P[2] + sb * eps_b
    pre = torch.einsum("sbk,snk->sbn", x, W) + b[:, None, :]
    y = torch.relu(pre) if c["relu"] else pre
    assert not bool((pre == 0).any())
    loss = (y * t(d["gy"])).sum()
    if kl == "kl":
        for s in range(S):
            lp = _log_prior(W[s], d["prior"]) + _log_prior(b[s], d["prior"])
            # log q at w = mu + sigma eps, with w - mu written as sigma eps: d log q / d mu = 0, d log q / d sigma = -1 / sigma.
            # (Formed as (mu + sigma eps) - mu, the two mu paths of autograd cancel only up to eps / sigma * 2^-53 -- 1e-11 at
            # rho = -12, this comparison's whole margin on a small element.)
            lq = _log_normal(sw * eps_w[s], 0.0, sw).sum() + _log_normal(sb * eps_b[s], 0.0, sb).sum()
            loss = loss + float(d["glp"][s]) * lp + float(d["glq"][s]) * lq
    loss.backward()
    inp = dict(d, y=y.detach().numpy(), x=x.detach().numpy())
    res = R.bbb_run(name, kl, want_bound=False, inputs=inp)
    got = res.grads
    assert c["math"] == "f32"
    gx = x.grad * ((x > 0).to(F64) if c["mask"] else 1.0)
    _rel_equal(got, (P[0].grad, P[1].grad, P[2].grad, P[3].grad, gx), name)


@pytest.mark.parametrize("kl", R.KL_MODES)
@pytest.mark.parametrize("name", ["lr-38", "lr-38-mem", "lr-odd", "lr-72-f32", "lr-out-n3"])
def test_lr_restatement_equals_autograd_in_fp64(name, kl):
    """m = x M, v = x^2 sigma^2, y = relu(m + sqrt(v) eps + b_mu + sigma_b eps_b), the closed-form KL against N(0, sigma_p^2);
    v handed to the restatement is the fp64 forward's (zero on the all-zero rows of x, where h = 0)."""
    c, d = R.LR_CASES[name], R.lr_inputs(name)
    S = c["S"]
    t = lambda a: torch.from_numpy(a).to(F64)
    x0 = t(d["x"]) if c["x3"] else t(d["x"]).unsqueeze(0).repeat(S, 1, 1)
    x = x0.clone().requires_grad_(True)
    P = [t(d[k]).clone().requires_grad_(True) for k in ("w_mu", "w_rho", "b_mu", "b_rho")]
    eps_act, eps_b = t(d["eps_act"][:S]), t(d["eps_b"][:S])
    sw, sb = torch.log1p(torch.exp(P[1])), torch.log1p(torch.exp(P[3]))
    v = torch.einsum("sbk,kn->sbn", x * x, sw * sw)
    live = (x0 != 0).any(2, keepdim=True).expand_as(v)               # sqrt has no gradient at 0: the rows with v == 0 take h = 0
    sd = torch.where(live, torch.sqrt(torch.where(live, v, torch.ones_like(v))), torch.zeros_like(v))
    pre = torch.einsum("sbk,kn->sbn", x, P[0]) + sd * eps_act + (P[2] + sb * eps_b)[:, None, :]
    y = torch.relu(pre) if c["relu"] else pre
    assert not bool((pre == 0).any())
    sp = d["sigma_p"]
    klf = lambda mu, sg: (math.log(sp) - torch.log(sg) + (sg ** 2 + mu ** 2) / (2 * sp ** 2) - 0.5).sum()
    loss = (y * t(d["gy"])).sum()
    if kl == "kl":
        kw, kb = klf(P[0], sw), klf(P[2], sb)
        g = [float(a) for a in d["gkl"]]
        loss = loss + g[0] * (kw + kb) + g[1] * kw + g[2] * kb
    loss.backward()
    res = R.lr_ref(x.detach(), d["gy"], y.detach(), v.detach(), d["w_mu"], d["w_rho"], d["b_mu"], d["b_rho"], sigma_p=sp,
                   relu=c["relu"], eps_act=eps_act, eps_b=eps_b, g_kl=d["gkl"] if kl == "kl" else None, gx_relu_mask=c["mask"],
                   want_bound=False)
    gx = x.grad * ((x > 0).to(F64) if c["mask"] else 1.0)
    _rel_equal(res.grads, (P[0].grad, P[1].grad, P[2].grad, P[3].grad, gx), name)


# ------------------------------------------------------------------------------------------ 2. fp32 inside the bound
@pytest.mark.parametrize("kl", R.KL_MODES)
@pytest.mark.parametrize("kind,name", ALL)
def test_fp32_restatement_lies_inside_the_bound(kind, name, kl):
    ref = _run(kind, name, kl)
    f32 = _run(kind, name, kl, dtype=torch.float32, want_bound=False)
    sh = R.shares(f32.grads, ref)
    print(f"{name:18s} {kl:4s} fp32 share of the bound: " + "  ".join(f"{n} {s:.3f}" for n, s in zip(R.NAMES, sh))
          + f"  ties {ref.info['tie_share']:.4f}")
    assert max(sh) <= 1.0, (name, kl, dict(zip(R.NAMES, sh)))
    assert ref.info["tie_share"] < 0.01
    for b in ref.bounds:
        assert bool(torch.isfinite(b).all())


@pytest.mark.parametrize("name", [n for n, c in R.BBB_CASES.items() if c["prior"] == "mix"])
def test_a_fifth_of_the_sampled_weights_lies_inside_three_sigma2(name):
    assert R.bbb_run(name, "kl").info["inside_3sigma2"] >= 0.20


def test_inputs_carry_the_edges():
    for name, c in R.BBB_CASES.items():
        d = R.bbb_inputs(name)
        if c["relu"]:
            z = d["y"] == 0
            assert (z.mean() > 0.03 or z.size < 500) and np.signbit(d["y"][z]).any() and not np.signbit(d["y"][z]).all()
            assert d["gy"][z].any()
        if c["S"] * c["B"] > 1:
            assert not d["gy"][0, 0].any()
        assert (d["x"] == 0).any()
    for name, c in R.LR_CASES.items():
        d = R.lr_inputs(name)
        assert not d["x"][..., 1:3, :].any() and not d["v"][:, 1:3].any() and not d["hfac"][:, 1:3].any()


# ------------------------------------------------------------------------------------------ 3. wrong variants break it
def _applies(kind, c, kl, variant):
    S, B, K, N = c["S"], c["B"], c["K"], c["N"]
    bf16 = c["math"] == "bf16"
    if kind == "lr":
        bf16 = R.lr_gx_bf16(bf16, N, B, c["eps"] == "philox" and c["mode"] == "v")
    return {
        "mask_ge": c["relu"],
        "drop_last_row": True,
        "clamp_last_k": K > 1,
        "clamp_last_feature": N > 1,
        "eps_next_sample": True,
        "eps_shift_group": True,
        "bias_no_q": kl == "kl",
        "no_factor_2": kind == "lr",
        "h_unguarded": kind == "lr" and c["mode"] == "v",
        "prior_at_mu": kind == "bbb" and kl == "kl",
        "mix_swapped": kind == "bbb" and kl == "kl" and c["prior"] == "mix",
        "gz_not_rounded": bf16,
    }[variant]


VARIANTS = ("mask_ge", "drop_last_row", "clamp_last_k", "clamp_last_feature", "eps_next_sample", "eps_shift_group", "bias_no_q",
            "no_factor_2", "h_unguarded", "prior_at_mu", "mix_swapped", "gz_not_rounded")


@pytest.mark.parametrize("kl", R.KL_MODES)
@pytest.mark.parametrize("kind,name", ALL)
def test_seeded_wrong_variants_break_the_bound(kind, name, kl):
    """mask y >= 0; last batch row left out; last k column / last feature from its clamped neighbour; epsilon of sample s + 1;
    epsilon shifted by one Philox group; -c / sigma dropped from the bias only; LR's factor 2 missing; h != 0 where v == 0
    (the unguarded quotient); the prior term at mu; the mixture's component weights swapped; gz not rounded in bf16 math."""
    c = (R.BBB_CASES if kind == "bbb" else R.LR_CASES)[name]
    ref = _run(kind, name, kl)
    line = []
    for variant in VARIANTS:
        if not _applies(kind, c, kl, variant):
            continue
        bad = _run(kind, name, kl, variant=variant, want_bound=False)
        worst = max(R.shares(bad.grads, ref))
        line.append(f"{variant} {worst:.2g}")
        assert worst > 1.0, (name, kl, variant, worst)
    print(f"{name:18s} {kl:4s} variants miss the bound by: " + "  ".join(line))
