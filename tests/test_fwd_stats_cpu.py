"""The fp64 restatement of the forward statistics (tests/fwd_stats_ref.py), its regime cells and its bound, proven without
a GPU:
 1. the restatement equals the oracle (oracle/bnn_oracle.py: bbb_linear, kl_closed_form, evaluated in float64) on every
    regular cell to 1e-12 relative -- log q up to the oracle's own (w - mu) cancellation, the KL up to the fp64 roundoff of
    its cancelling components, both derived in the module;
 2. the reference's own fp32 formula and an fp32 emulation of the kernels' arithmetic (exact exp2 / log2, denormals kept and
    flushed) lie inside the bound on every regular cell: the bound is a condition on the INPUTS, not on one implementation;
 3. the cells are what the module says: 96 regular, 2 band, 3 edge per prior, judged by the reference's fp32 formula;
 4. six seeded wrong variants of the emulation -- each a plausible kernel slip -- and which of them the suite's init-range
    sums (rtol 2e-5 on log q / log p, 2e-6 on the KL and its sums, at mu +-0.2, rho in [-5, -4]) would have caught."""
import math

import numpy as np
import pytest
import torch

import fwd_stats_ref as R
from oracle import bnn_oracle as O

N, K, B, S = 16, 8, 16, 4
REL = 1e-12


def _inputs(cell):
    w_mu, w_rho, b_mu, b_rho = R.cell_params(cell, N, K)
    eps_w, eps_b = R.cell_eps(S, N, K)
    return w_mu, w_rho, b_mu, b_rho, eps_w, eps_b


@pytest.fixture(scope="module")
def refs():
    """fp64 statistics of every cell of every prior, computed once."""
    x = R.cell_x(B, K)
    return {c.name: R.bbb_ref(x, *_inputs(c), R.PRIORS[p]) for p in R.PRIORS for c in R.cells(p)}


# ------------------------------------------------------------------------------------------ 1. restatement == the oracle
@pytest.mark.parametrize("prior", list(R.PRIORS))
def test_restatement_equals_the_oracle_in_fp64(prior, refs):
    pr = R.PRIORS[prior]
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    x = R.cell_x(B, K)
    worst = dict(lq=0.0, lp=0.0, y=0.0)
    for c in R.cells(prior):
        if c.tag != "regular":
            continue
        w_mu, w_rho, b_mu, b_rho, eps_w, eps_b = _inputs(c)
        ref = refs[c.name]
        slack = R.oracle_lq_slack(w_mu, w_rho, b_mu, b_rho, eps_w, eps_b)
        tags = R.prior_sample_tags(pr, ref.m)
        for s in range(S):
            y, lp, lq = O.bbb_linear(t(x), t(w_mu), t(w_rho), t(b_mu), t(b_rho), t(eps_w[s]), t(eps_b[s]),
                                     O.Prior(pr.mixture, pr.sigma_p, pr.pi, pr.sigma1, pr.sigma2))
            e = abs(float(lq) - ref.log_q[s])
            assert e <= REL * abs(ref.log_q[s]) + slack[s], (c.name, s, e)
            worst["lq"] = max(worst["lq"], (e - slack[s]) / abs(ref.log_q[s]))
            if tags[s] == "regular":
                e = abs(float(lp) - ref.log_prior[s])
                assert e <= REL * abs(ref.log_prior[s]), (c.name, s, e, ref.log_prior[s])
                worst["lp"] = max(worst["lp"], e / abs(ref.log_prior[s]))
            cond = np.abs(x) @ np.abs(ref.w[s]).T + np.abs(ref.bias[s])
            e = np.abs(y.numpy() - ref.y[s])
            assert bool(np.all(e <= REL * cond)), (c.name, s)
            worst["y"] = max(worst["y"], float((e / np.maximum(cond, 1e-300)).max()))
    print(f"{prior}: largest relative difference from the oracle  " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()))


@pytest.mark.parametrize("name", list(R.LR_SIGMA_P))
def test_kl_restatement_equals_the_oracle_in_fp64(name):
    sp = R.LR_SIGMA_P[name]
    for c in R.lr_cells(name):
        if c.tag != "regular":
            continue
        w_mu, w_rho, b_mu, b_rho = R.cell_params(c, N, K, lr=True)
        mu, rho = np.concatenate([w_mu.ravel(), b_mu]), np.concatenate([w_rho.ravel(), b_rho])
        kl, ls, s2, m2 = R.kl_ref(mu, rho, sp).value
        t = lambda a: torch.from_numpy(a.astype(np.float64))
        want = float(O.kl_closed_form(t(mu), O.softplus_naive(t(rho)), 0.0, sp))
        # fp64 roundoff of the components that cancel (2 n log sp against 2 ls against n against the quadratic terms)
        cond = 2 * mu.size * abs(math.log(sp)) + 2 * abs(ls) + mu.size + (s2 + m2) / sp ** 2
        assert abs(kl - want) <= REL * abs(want) + 8 * 2.0 ** -53 * cond, (c.name, kl, want)


# ---------------------------------------------------------------------- 2. the bound is a condition on the inputs
@pytest.mark.parametrize("prior", list(R.PRIORS))
def test_reference_formula_and_emulation_lie_inside_the_bound(prior, refs):
    pr = R.PRIORS[prior]
    worst = {}
    n_reg = 0
    for c in R.cells(prior):
        if c.tag != "regular":
            continue
        inp = _inputs(c)
        ref = refs[c.name]
        reg = np.array([tg == "regular" for tg in R.prior_sample_tags(pr, ref.m)])
        assert reg[0] == (not pr.mixture or c.mu <= R.MU_TOP * R.wide_scale(pr) * (1 + 1e-9)), c.name
        n_reg += int(reg.sum())
        runs = {"reference": R.reference_fp32(*inp, pr), "emulation": R.emu_bbb(*inp, pr),
                "emulation, flushed": R.emu_bbb(*inp, pr, flush=True)}
        for what, (lq, lp) in runs.items():
            own = R.reference_slack(*inp, pr) if what == "reference" else (0.0, np.zeros(S))
            sh = (R.share(lq, ref.log_q, ref.b_log_q + own[0]), R.share(lp[reg], ref.log_prior[reg], (ref.b_log_prior + own[1])[reg]))
            assert max(sh) <= 1.0, (c.name, what, sh)
            worst[what] = tuple(max(a, b) for a, b in zip(worst.get(what, (0.0, 0.0)), sh))
    assert n_reg >= 96
    for what, sh in worst.items():
        print(f"{prior:14s} {what:20s} largest share of the bound: log_q {sh[0]:.3f}  log_prior {sh[1]:.3f}")


@pytest.mark.parametrize("name", list(R.LR_SIGMA_P))
def test_kl_reference_formula_and_emulation_lie_inside_the_bound(name):
    sp = R.LR_SIGMA_P[name]
    worst = np.zeros(5)
    for c in R.lr_cells(name):
        if c.tag != "regular":
            continue
        for n in (1, 7, 1027, None):
            if n is None:
                w_mu, w_rho, b_mu, b_rho = R.cell_params(c, N, K, lr=True)
                mu, rho = np.concatenate([w_mu.ravel(), b_mu]), np.concatenate([w_rho.ravel(), b_rho])
            else:
                mu, rho = R.cell_params(c, 1, n)[:2]
            ref = R.kl_ref(mu, rho, sp)
            sh = [R.share(R.reference_kl_fp32(mu, rho, sp), ref.value[0], ref.bound[0])]
            for flush in (False, True):
                got = R.emu_kl(mu, rho, sp, flush=flush)
                sh2 = [R.share(g, v, b) for g, v, b in zip(got, ref.value, ref.bound)]
                assert max(sh2) <= 1.0, (c.name, n, flush, sh2)
                sh = sh + sh2 if not flush else sh
            assert sh[0] <= 1.0, (c.name, n, sh)
            worst = np.maximum(worst, sh)
    print(f"{name}: largest share  reference KL {worst[0]:.3f}  emulation kl {worst[1]:.3f} ls {worst[2]:.3f} s2 {worst[3]:.3f} m2 {worst[4]:.3f}")


# ------------------------------------------------------------------------------------------------- 3. the cells
@pytest.mark.parametrize("prior", list(R.PRIORS))
def test_cell_classification(prior, refs):
    pr = R.PRIORS[prior]
    cs = R.cells(prior)
    tags = [c.tag for c in cs]
    assert (tags.count("regular"), tags.count("band"), tags.count("edge")) == (96, 2, 3)
    assert len({c.name for c in cs}) == len(cs)
    s1 = R.wide_scale(pr)
    for c in cs:
        w_mu, w_rho, b_mu, b_rho, eps_w, eps_b = _inputs(c)
        rho, amu = np.concatenate([w_rho.ravel(), b_rho]), np.abs(np.concatenate([w_mu.ravel(), b_mu]))
        # every parameter in the cell's neighbourhood
        assert np.all(np.abs(rho - c.rho) <= max(0.02 * abs(c.rho), 0.02) * (1 + 1e-6)), c.name
        assert np.all(np.abs(amu - c.mu) <= 0.02 * c.mu * (1 + 1e-6)), c.name
        assert c.mu == 0 or (np.any(w_mu > 0) and np.any(w_mu < 0)), c.name
        lq, lp = R.reference_fp32(w_mu, w_rho, b_mu, b_rho, eps_w, eps_b, pr)
        m = refs[c.name].m
        ptags = R.prior_sample_tags(pr, m)
        if c.tag == "regular":
            # exactly: rho in [-20, 80] and, for the log prior, |w| <= 12.5 sigma1
            assert -20.4 <= rho.min() and rho.max() <= 81.6 and np.all(np.isfinite(lq)), c.name
            assert ptags[0] == "regular" if not pr.mixture else np.all(amu <= R.MU_TOP * s1) == (ptags[0] == "regular"), c.name
            for s in range(S):
                if ptags[s] == "regular":
                    assert np.isfinite(lp[s]), (c.name, s)
                elif ptags[s] == "beyond":
                    assert not np.isfinite(lp[s]), (c.name, s)
        elif c.tag == "band":
            # finite in the reference, whose exp and log keep denormals: sigma a non-zero denormal with a finite logarithm (its
            # log q is NaN all the same -- sigma^2 underflows under (w - mu)^2 = 0); the density of the wide component likewise
            sg = torch.log1p(torch.exp(torch.from_numpy(rho)))
            if c.rho == R.RHO_BAND:
                assert bool(((sg > 0) & (sg < 2.0 ** -126)).all()) and bool(torch.isfinite(torch.log(sg)).all()), c.name
            else:
                assert np.all(np.isfinite(lq)) and np.isfinite(lp[0]) and (not pr.mixture or ptags[0] == "band"), c.name
        else:
            if c.rho in R.RHO_EDGES:
                assert not np.any(np.isfinite(lq)), c.name
            else:
                assert np.all(np.isfinite(lq)), c.name
                assert np.isfinite(lp[0]) == (not pr.mixture), c.name        # a Gauss prior has no exponential to underflow
                assert not pr.mixture or ptags[0] == "beyond", c.name


def _finite_limit(fn, pr):
    """Largest |w| / sigma1 (to 0.01) at which fn's mixture log prior of a single weight w is finite."""
    lo, hi = 1.0, 40.0
    z = np.zeros((1, 1), np.float32)
    while hi - lo > 0.005:
        mid = 0.5 * (lo + hi)
        w = np.full((1, 1), mid * R.wide_scale(pr), np.float32)
        lp = fn(w, z - 200.0, z[0], z[0] - 200.0, z[None], z, pr)[1]          # rho = -200: w = mu; the bias sits at 0
        lo, hi = (mid, hi) if np.isfinite(lp[0]) else (lo, mid)
    return lo


@pytest.mark.parametrize("prior", R.NONDEGENERATE_MIX)
def test_the_denormal_band_is_where_the_cells_put_it(prior):
    """The reference (denormals kept) is finite past the band cell, an emulation that flushes them stops short of it, and
    both agree on the regular side (12.5 sigma1) and on the edge (15 sigma1)."""
    pr = R.PRIORS[prior]
    ref = _finite_limit(R.reference_fp32, pr)
    keep = _finite_limit(lambda *a: R.emu_bbb(*a), pr)
    flush = _finite_limit(lambda *a: R.emu_bbb(*a, flush=True), pr)
    print(f"{prior}: finite up to |w| / sigma1 = {ref:.2f} (reference)  {keep:.2f} (emulation)  {flush:.2f} (emulation, flushed)")
    assert R.MU_TOP * 1.001 < flush < R.MU_BAND * 0.98 and R.MU_BAND * 1.02 < ref < R.MU_EDGE * 0.98
    assert R.MU_BAND * 1.02 < keep < R.MU_EDGE * 0.98


def test_the_abi_accepts_pi_one():
    """pi = 1 is a legal bnn_prior (the wide component alone): the cells include it; nothing refuses it on the way in."""
    from bnn_hip import ops
    p = ops.PriorSpec(True, 1.0, 1.0, 1.0, math.exp(-6.0)).c()
    assert p.pi == 1.0 and p.sigma1 == 1.0


# ------------------------------------------------------------------------------------------ 4. seeded wrong variants
def _init_range_catches(variant):
    """Would the suite's init-range sums have caught it?  mu in +-0.2, rho in [-5, -4], 10^4 weights, one N(0, 1) sample:
    log q / log p at rtol 2e-5 (Gauss 1.0 and the mixture (0.5, 1, e^-6)), the KL and its sums at rtol 2e-6."""
    rs = np.random.RandomState(5)
    n = 10000
    mu, rho = rs.uniform(-0.2, 0.2, (1, n)).astype(np.float32), rs.uniform(-5, -4, (1, n)).astype(np.float32)
    bm, br = mu[0, :1].copy(), rho[0, :1].copy()
    ew, eb = rs.standard_normal((1, 1, n)).astype(np.float32), rs.standard_normal((1, 1)).astype(np.float32)
    caught = []
    for pn in ("gauss-1", "mix-0.5-0-6"):
        pr = R.PRIORS[pn]
        ref = R.bbb_ref(np.zeros((1, n)), mu, rho, bm, br, ew, eb, pr)
        lq, lp = R.emu_bbb(mu, rho, bm, br, ew, eb, pr, variant=variant)
        caught += [abs(lq[0] - ref.log_q[0]) > 2e-5 * abs(ref.log_q[0]), abs(lp[0] - ref.log_prior[0]) > 2e-5 * abs(ref.log_prior[0])]
    ref = R.kl_ref(mu, rho, 1.0).value
    got = R.emu_kl(mu, rho, 1.0, variant=variant)
    caught += [abs(g - v) > 2e-6 * abs(v) for g, v in zip(got, ref)]
    return any(caught)


def _largest_share(variant):
    worst, where = 0.0, None
    if variant in ("softplus_no_residue", "mix_no_inv_sigma", "mix_drop_narrow", "logq_sigma_bf16"):
        for p in R.PRIORS:
            pr = R.PRIORS[p]
            if variant.startswith("mix") and p not in R.NONDEGENERATE_MIX:
                continue
            x = R.cell_x(B, K)
            for c in R.cells(p):
                if c.tag != "regular":
                    continue
                inp = _inputs(c)
                ref = R.bbb_ref(x, *inp, pr)
                reg = np.array([tg == "regular" for tg in R.prior_sample_tags(pr, ref.m)])
                lq, lp = R.emu_bbb(*inp, pr, variant=variant)
                sh = max(R.share(lq, ref.log_q, ref.b_log_q), R.share(lp[reg], ref.log_prior[reg], ref.b_log_prior[reg]))
                if sh > worst:
                    worst, where = sh, c.name
    if not variant.startswith("mix"):
        for name, sp in R.LR_SIGMA_P.items():
            for c in R.lr_cells(name):
                if c.tag != "regular":
                    continue
                w_mu, w_rho, b_mu, b_rho = R.cell_params(c, N, K, lr=True)
                mu, rho = np.concatenate([w_mu.ravel(), b_mu]), np.concatenate([w_rho.ravel(), b_rho])
                ref = R.kl_ref(mu, rho, sp)
                got = R.emu_kl(mu, rho, sp, variant=variant)
                sh = max(R.share(g, v, b) for g, v, b in zip(got, ref.value, ref.bound))
                if sh > worst:
                    worst, where = sh, c.name
    return worst, where


@pytest.mark.parametrize("variant", [v for v in R.VARIANTS if v != "kl_fp32_combine"])
def test_seeded_wrong_variants_break_the_bound(variant):
    """(a) softplus without the residue, (b) mixture weights without 1 / sigma_i, (c) the narrow component dropped, (d) sigma^2
    rounded to bf16 before the KL's sum, (f) sum log sigma from a bf16 sigma: each exceeds the bound in a regular cell."""
    worst, where = _largest_share(variant)
    print(f"{variant}: largest share of the bound {worst:.3g} at {where}; the init-range sums "
          f"{'would have caught it' if _init_range_catches(variant) else 'do NOT catch it'}")
    assert worst > 1.0, (variant, worst, where)


def test_softplus_emulation_over_the_probe_range():
    """The emulated bnn::softplus stays within (E_SP + A_RHO |rho|) u over the probe range of E_SP; with the residue added at
    every e -- the kernels' softplus until the probe was widened past rho = 2 -- it is off by tens of u wherever 1 + e crosses
    a binade and by up to 12 % in rho [16.64, 17.33)."""
    rho = R.softplus_probe_points()
    now, before = R.softplus_rest_in_u(R.emu_softplus(rho), rho), R.softplus_rest_in_u(R.emu_softplus(rho, residue_limit=False), rho)
    print(f"emulated softplus over [-20, 80]: rest beyond {R.A_RHO} |rho| u: {now:.3f} u; with the unlimited residue {before:.3g} u")
    assert now <= R.E_SP / 2 and before > 1e5
    x = np.array([88.6, 88.7, 88.8, 89.0], np.float32)            # finite up to the overflow of exp, +inf from there
    got = R.emu_softplus(x)
    assert np.all(np.abs(got[:2] - x[:2]) <= 1e-4) and np.all(np.isposinf(got[2:]))


def test_fp32_combine_of_the_kl_is_inside_any_sound_bound():
    """(e) the KL combined in fp32 from the three sums, in the cancelling order.  Its error is three roundings of the largest
    intermediate, <= 3 u (2 n |log sp| + 2 |ls| + n + (s2 + m2) / sp^2); the sums it starts from are themselves only known to
    (E + n) u of the same magnitudes (v_log_f32, softplus, any-order summation), so no bound that admits every correct
    kernel can exclude it, at the cancellation cell or anywhere else: an ABSOLUTE bound makes (e) harmless (KL ~ 0 there is
    then right to n u), where the relative check it replaces would have been meaningless.  Asserted as that: inside the
    bound in every regular cell, with a relative error that no rtol would pass at the cancellation cell."""
    worst, where = _largest_share("kl_fp32_combine")
    print(f"kl_fp32_combine: largest share of the bound {worst:.3g} at {where}; the init-range sums "
          f"{'would have caught it' if _init_range_catches('kl_fp32_combine') else 'do NOT catch it'}")
    assert worst <= 1.0
    rel = []
    for name, sp in R.LR_SIGMA_P.items():
        c = [c for c in R.lr_cells(name) if c.name.endswith("/cancel")][0]
        mu, rho = R.cell_params(c, 1, 1027)[:2]
        ref = R.kl_ref(mu, rho, sp)
        got = R.emu_kl(mu, rho, sp, variant="kl_fp32_combine")
        rel.append(abs(got[0] - ref.value[0]) / abs(ref.value[0]))
        assert abs(got[0] - ref.value[0]) <= ref.bound[0]
    print("kl_fp32_combine at the cancellation cells, n = 1027: relative error of the KL " + "  ".join(f"{r:.1e}" for r in rel))
