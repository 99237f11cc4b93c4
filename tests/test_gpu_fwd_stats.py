"""The forward statistics -- log q(w), log p(w) under the Gaussian and the scale-mixture prior, the closed-form KL and its
three sums, the fp32 y -- of every kernel that restates them, on an MI355X against the fp64 restatement
tests/fwd_stats_ref.py, regime cell by regime cell (that module's docstring: the cells, the bound and its derivation;
tests/test_fwd_stats_cpu.py proves the restatement against the oracle, the bound wide enough for the reference's formula and
tight enough for seeded wrong variants).  One launch per cell, every weight of it in one (prior, rho, |mu|) regime:
  regular cells   every statistic within its bound;
  edge cells      rho = 89 (sigma = +inf), rho = -200 (sigma = 0), |mu| = 15 sigma1: every statistic the edge reaches is
                  non-finite (sign and NaN-ness free); y at rho = 89 non-finite, elsewhere within its bound;
  band cells      rho = -100 (sigma a denormal), |mu| = 13.6 sigma1 (the wide component's density a denormal): within the
                  bound, or what a flushed denormal gives (-+inf); which one is printed.
Entry points: bbb_linear_fwd as K1a (tile form; fp32, bf16 and split-bf16 math, ragged shape), K1b / K1b2 (block GEMM without
and with a hoisted sigma; injected epsilon, and on-chip epsilon from ops.philox_normal), the K-sliced form, the split-bf16 block form; K1s
(bbb_sample_weights + elbo_finalize); flipout_prepare; sparse_elbo_terms at two pruning levels; bbb_group_train's loss_info;
gauss_kl; lr_linear_fwd's fused KL in tile and block form; lr_prepare's workspace KL through elbo_finalize; eval_prepare's
sigma.  K1b2 needs at least four (sample, batch block) units, so its cases run S = 5 (an odd number of units: the last
block's second pair slot is idle) where K1b runs S = 3.

Measured on the MI355X: v_exp_f32 1.257 u (E_EXP = 4), fast_log 2.165 u max(|log sigma|, 1) (E_LOG = 8), ops.softplus 2.778 u beyond
1.25 |rho| u over [-20, 80] (E_SP = 8; 15.4 u at its worst, rho = -16.6).  Before this file bnn::softplus added its rounding
residue at every e: the same probe read 2.0e6 u (sigma off by 12 %) at rho = 16.65; csrc/bnn_device.h now stops it at e = 1.
Both bands FLUSH on the device, in every entry point: rho = -100 gives sigma = 0, log q = +inf, KL = +inf (weight_kl = kl -
bias_kl = NaN); |w| = 13.6 sigma1 gives log p = -inf.  Every edge cell is non-finite where the edge reaches.
Nothing but the three constants was tuned on the device's figures; largest share of the bound over the regular cells,
afterwards (Gauss priors | mixtures):
                            log_q          log_prior      y
  K1a fp32 (8,16,16,4)      0.073 | 0.074  0.448 | 0.041  0.243 | 0.258
  K1a fp32 (33,7,5,3)       0.055 | 0.053  0.255 | 0.029  0.069 | 0.074
  K1a bf16, both shapes     as fp32 (the statistics come from the un-rounded fp32 weights)
  K1a split-bf16            0.073 | 0.074  0.440 | 0.084
  K1b (8,16,16,3)           0.073 | 0.074  0.440 | 0.084
  K1b (72,40,16,3)          0.031 | 0.030  0.335 | 0.002
  K1b2 (8,16,16,5)          0.073 | 0.074  0.460 | 0.028      (the split-bf16 block form: the same)
  K1b2 (72,40,16,5)         0.031 | 0.030  0.332 | 0.002
  K1b / K1b2 on-chip eps    0.002 | 0.002  0.367 | 0.002
  K-sliced (104,16,16,3)    0.038 | 0.037  0.296 | 0.003
  K1s + finalize            0.023 | 0.023  0.480 | 0.063      sampled bias 0.995 (half an ulp of fma(sigma, eps, mu))
  flipout_prepare           0.073 | 0.078  0.448 | 0.041
  sparse, half kept         0.029 | 0.026  0.442 | 0.120
  sparse, an eighth kept    0.045 | 0.049  0.277 | 0.075
  bbb_group (means)         0.009 | 0.009  0.157 | 0.010
                            kl     ls     s2     m2
  gauss_kl n = 1            0.096  0.125  0.367  0.044
  gauss_kl n = 7            0.069  0.070  0.227  0.073
  gauss_kl n = 1027         0.007  0.025  0.010  0.002
  lr_linear_fwd, 3 forms    0.022  (bias_kl 0.052, weight_kl 0.021)        lr_prepare + finalize 0.022
  eval_prepare's sigma      0.693
(0.5, 1, 1) against Gauss 1: 0.010 of the two bounds.
"""
import collections
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fwd_stats_ref as R
from bnn_hip import _lib as L
from bnn_hip import ops

SEED, LAYER_ID, OFFSET = 0x5EEDF00D12345678, 1, 3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _stop_on_a_device_error():
    """An assertion that fails lets the next test run; an error of the device ends the session."""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as exc:                                   # noqa: BLE001
        pytest.exit(f"device error: {exc}", returncode=3)


def _up(a, dev):
    return None if a is None else (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(dev)


def _spec(pr):
    return ops.PriorSpec(pr.mixture, pr.sigma_p, pr.pi, pr.sigma1, pr.sigma2)


@functools.lru_cache(maxsize=None)
def _dev_eps(S, N, K, dev):
    ew, eb = R.cell_eps(S, N, K)
    return _up(ew, dev), _up(eb, dev)


@functools.lru_cache(maxsize=None)
def _philox(S, N, K, dev, seed=SEED, layer_id=LAYER_ID, first=OFFSET):
    """(eps_w [S, N, K], eps_b [S, N]) of the on-chip stream (ops.philox_normal is bit-pinned to the CPU restatement)."""
    ew = ops.philox_normal(seed, 4 * layer_id + 0, first, S, N, K, dev).cpu().numpy()
    eb = ops.philox_normal(seed, 4 * layer_id + 1, first, S, 1, N, dev).cpu().numpy().reshape(S, N)
    return ew, eb


class Tally:
    """Largest share of the bound per statistic over a test's regular cells, and what the band cells did."""

    def __init__(self, what):
        self.what, self.sh, self.band = what, collections.OrderedDict(), collections.OrderedDict()

    def add(self, name, sh, where):
        assert sh <= 1.0, (self.what, name, where, sh)
        self.sh[name] = max(self.sh.get(name, 0.0), sh)

    def note(self, name, flushed):
        self.band.setdefault(name, set()).add("flushed" if flushed else "within the bound")

    def report(self):
        print(f"{self.what:34s} share of the bound: " + "  ".join(f"{k} {v:.3f}" for k, v in self.sh.items())
              + "".join(f"  | band {k}: {' and '.join(sorted(v))}" for k, v in self.band.items()))


def judge_rho(t, c, name, got, ref, bound, difference=False):
    """A statistic whose regime is rho alone (log q, sum log sigma, the KL, sum sigma^2).  `difference`: formed as the
    difference of two such statistics, so inf - inf = NaN where both are flushed."""
    got, ref, bound = (np.atleast_1d(np.asarray(a, np.float64)) for a in (got, ref, bound))
    if c.rho in R.RHO_EDGES:
        assert not np.isfinite(got).any(), (t.what, c.name, name, got)
    elif c.rho == R.RHO_BAND:
        for g, r, b in zip(got, ref, bound):
            assert np.isinf(g) or (difference and np.isnan(g)) or abs(g - r) <= b, (t.what, c.name, name, g, r, b)
            t.note(name, not np.isfinite(g))
    else:
        t.add(name, R.share(got, ref, bound), c.name)


def judge_log_prior(t, c, pr, got, ref, bound, m, name="log_prior"):
    """Per sample, by the regime its sampled weights reach (fwd_stats_ref.prior_sample_tags)."""
    got = np.atleast_1d(np.asarray(got, np.float64))
    if c.rho == 89.0:
        assert not np.isfinite(got).any(), (t.what, c.name, name, got)
        return
    for s, tag in enumerate(R.prior_sample_tags(pr, m)):
        if tag == "regular":
            t.add(name, R.share(got[s], ref[s], bound[s]), (c.name, s))
        elif tag == "band":
            assert (np.isinf(got[s]) and got[s] < 0) or abs(got[s] - ref[s]) <= bound[s], (t.what, c.name, s, got[s], ref[s], bound[s])
            if c.tag == "band":
                t.note(name, bool(np.isinf(got[s])))
        elif tag == "beyond":
            assert not np.isfinite(got[s]), (t.what, c.name, name, s, got[s])


def judge_y(t, c, got, ref, bound):
    if c.rho == 89.0:
        assert not np.isfinite(got).any(), (t.what, c.name, "y")
    else:
        t.add("y", R.share(got, ref, bound), c.name)


# ------------------------------------------------------------------------------------------------- the measured constants
def test_transcendental_error_constants(dev):
    """E_SP, E_EXP, E_LOG of tests/fwd_stats_ref.py, re-measured against fp64: each at most half its constant.  (The probe of
    test_gpu_layer_bwd.test_softplus_error_constant, [-12, 2], stays where it is; this one covers [-20, 80] and the two units.)"""
    rho = R.softplus_probe_points()
    got = ops.softplus(_up(rho, dev)).cpu().numpy()
    e_sp = R.softplus_rest_in_u(got, rho)
    err = np.abs(got.astype(np.float64) - R.softplus64(rho)) / (R.U * R.softplus64(rho))
    print(f"softplus over [-20, 80]: largest relative error {err.max():.3f} u at rho = {rho[err.argmax()]:.3f}; "
          f"rest beyond {R.A_RHO} |rho| u: {e_sp:.3f} u (recorded {R.E_SP_MEASURED}, E_SP = {R.E_SP})")
    rho = R.exp_probe_points()
    got = ops.softplus(_up(rho, dev)).cpu().numpy()
    e_exp = R.exp_error_in_u(got, rho)
    print(f"v_exp_f32 over 2^[-125.5, -25.2]: largest relative error {e_exp:.3f} u (recorded {R.E_EXP_MEASURED}, E_EXP = {R.E_EXP})")
    rho = _up(R.log_probe_points(), dev)
    sigma = ops.softplus(rho)
    zero = torch.zeros(1, device=dev)
    got = torch.stack([ops.gauss_kl(zero, rho[i:i + 1], 1.0)[1] for i in range(rho.numel())]).cpu().numpy()
    e_log = R.log_error_in_u(got, sigma.cpu().numpy())
    print(f"fast_log over sigma in [2e-9, 80]: largest error {e_log:.3f} u max(|log sigma|, 1) (recorded {R.E_LOG_MEASURED}, E_LOG = {R.E_LOG})")
    assert e_sp <= R.E_SP / 2 and e_exp <= R.E_EXP / 2 and e_log <= R.E_LOG / 2, (e_sp, e_exp, e_log)


# ------------------------------------------------------------------------------------------------------ bbb_linear_fwd
def _e(K, N, B, S, form, math, **kw):
    return dict(K=K, N=N, B=B, S=S, form=form, math=math, sigma=False, eps="memory", **kw)


BBB = collections.OrderedDict([
    ("k1a-f32",         _e(8, 16, 16, 4, L.FORM_TILE, L.MATH_F32)),
    ("k1a-f32-ragged",  _e(33, 7, 5, 3, L.FORM_TILE, L.MATH_F32)),
    ("k1a-bf16",        _e(8, 16, 16, 4, L.FORM_TILE, L.MATH_BF16)),
    ("k1a-bf16-ragged", _e(33, 7, 5, 3, L.FORM_TILE, L.MATH_BF16)),
    ("k1a-x3",          _e(8, 16, 16, 3, L.FORM_TILE, L.MATH_BF16X3)),
    ("k1b",             _e(8, 16, 16, 3, L.FORM_GEMM, L.MATH_BF16)),
    ("k1b-k72",         _e(72, 40, 16, 3, L.FORM_GEMM, L.MATH_BF16)),
    ("k1b2",            dict(_e(8, 16, 16, 5, L.FORM_GEMM, L.MATH_BF16), sigma=True)),
    ("k1b2-k72",        dict(_e(72, 40, 16, 5, L.FORM_GEMM, L.MATH_BF16), sigma=True)),
    # on-chip epsilon, nothing dumped: with a Gauss prior the k-steps before the last whole one run K1b2's straight-line bodies
    ("k1b2-philox-k72", dict(_e(72, 40, 16, 5, L.FORM_GEMM, L.MATH_BF16), sigma=True, eps="philox")),
    ("k1b-philox-k72",  dict(_e(72, 40, 16, 3, L.FORM_GEMM, L.MATH_BF16), eps="philox")),
    ("k1b2-x3",         dict(_e(8, 16, 16, 5, L.FORM_GEMM, L.MATH_BF16X3), sigma=True)),
    ("kslice",          _e(104, 16, 16, 3, L.FORM_GEMM_KSLICE, L.MATH_BF16)),   # four k-steps: the fewest that split in two
])


def _bbb_launch(e, c, pr, dev, prior=None, plan_only=False):
    K, N, B, S = e["K"], e["N"], e["B"], e["S"]
    w_mu, w_rho, b_mu, b_rho = (_up(a, dev) for a in R.cell_params(c, N, K))
    x = _up(R.cell_x(B, K), dev)
    kw = dict(n_samples=S, prior=_spec(prior or pr), math_mode=e["math"], relu=False, y_dtype=torch.float32, seed=SEED,
              layer_id=LAYER_ID, sample_offset=OFFSET, want_stats=True, want_scalars=True, form=e["form"])
    if e["eps"] == "memory":
        ew, eb = _dev_eps(S, N, K, dev)
        kw.update(eps_mode=L.EPS_MEMORY, eps_w=ew, eps_b=eb)
    else:
        kw.update(eps_mode=L.EPS_PHILOX)
    if e["form"] != L.FORM_TILE:
        xf = x
        x = xf.to(torch.bfloat16)
        if e["math"] == L.MATH_BF16X3:
            kw["x_lo"] = (xf - x.float()).to(torch.bfloat16)
    elif e["math"] == L.MATH_BF16:
        x = x.to(torch.bfloat16)
    if e["sigma"]:
        kw["w_sigma"] = ops.softplus(w_rho)
    if e["form"] == L.FORM_GEMM_KSLICE:
        kw["split_scratch"] = ops.split_scratch_cached(S, B, N, dev)
    if plan_only:
        return ops.bbb_plan(x, w_mu, w_rho, b_mu, b_rho, **kw)
    return ops.bbb_linear_fwd(x, w_mu, w_rho, b_mu, b_rho, **kw)


def _check_plan(name, e, plan):
    pairs = e["S"] * ((e["B"] + 127) // 128)
    assert plan["form"] == e["form"], (name, plan)
    if e["form"] == L.FORM_GEMM:
        assert plan["waves"] == (8 if e["sigma"] else 4), (name, plan)
        assert not e["sigma"] or (pairs % 2 == 1 and plan["blocks"] == ((e["N"] + 63) // 64) * ((pairs + 1) // 2)), (name, plan)
    if e["form"] == L.FORM_GEMM_KSLICE:
        assert plan["k_slices"] >= 2, (name, plan)


def _bbb_ref(e, c, pr, dev):
    K, N, B, S = e["K"], e["N"], e["B"], e["S"]
    ew, eb = R.cell_eps(S, N, K) if e["eps"] == "memory" else _philox(S, N, K, dev)
    return R.bbb_ref(R.cell_x(B, K), *R.cell_params(c, N, K), ew, eb, pr)


@pytest.mark.parametrize("prior", list(R.PRIORS))
@pytest.mark.parametrize("name", list(BBB))
def test_bbb_linear_fwd_statistics_cell_by_cell(dev, name, prior):
    e, pr = BBB[name], R.PRIORS[prior]
    t = Tally(f"{name} {prior}")
    cs = R.cells(prior)
    _check_plan(name, e, _bbb_launch(e, cs[0], pr, dev, plan_only=True))
    for c in cs:
        out = _bbb_launch(e, c, pr, dev)
        ref = _bbb_ref(e, c, pr, dev)
        judge_rho(t, c, "log_q", out["log_q"].cpu().numpy(), ref.log_q, ref.b_log_q)
        judge_log_prior(t, c, pr, out["log_prior"].cpu().numpy(), ref.log_prior, ref.b_log_prior, ref.m)
        y = out["y"].cpu().numpy()
        if e["math"] == L.MATH_F32:
            judge_y(t, c, y, ref.y, ref.b_y)
        elif c.rho == 89.0:
            assert not np.isfinite(y).any(), (name, c.name)
    t.report()


@pytest.mark.parametrize("name", ["k1a-f32", "k1b2"])
def test_equal_components_match_the_gauss_prior(dev, name):
    """(0.5, 1, 1): both components N(0, 1).  The mixture path's log prior equals the Gauss path's within the two bounds."""
    e, mix, gauss = BBB[name], R.PRIORS["mix-equal"], R.PRIORS["gauss-1"]
    worst = 0.0
    for c in R.cells("mix-equal"):
        if c.tag != "regular":
            continue
        a, b = _bbb_launch(e, c, mix, dev), _bbb_launch(e, c, mix, dev, prior=gauss)
        ew, eb = R.cell_eps(e["S"], e["N"], e["K"])
        p = R.cell_params(c, e["N"], e["K"])
        ra, rb = R.bbb_ref(R.cell_x(e["B"], e["K"]), *p, ew, eb, mix), R.bbb_ref(R.cell_x(e["B"], e["K"]), *p, ew, eb, gauss)
        reg = np.array([tg == "regular" for tg in R.prior_sample_tags(mix, ra.m)])
        assert np.all(np.abs(ra.log_prior - rb.log_prior)[reg] <= 1e-12 * np.abs(rb.log_prior)[reg])
        d = np.abs(a["log_prior"].cpu().numpy().astype(np.float64) - b["log_prior"].cpu().numpy())[reg]
        sh = float((d / (ra.b_log_prior + rb.b_log_prior)[reg]).max())
        assert sh <= 1.0, (name, c.name, sh)
        worst = max(worst, sh)
    print(f"{name}: mixture (0.5, 1, 1) against Gauss 1: largest share of the two bounds {worst:.3f}")


# --------------------------------------------------------------------------- K1s, Flipout, the sparse step, the agent group
@pytest.mark.parametrize("prior", list(R.PRIORS))
def test_sampler_statistics_cell_by_cell(dev, prior):
    """K1s (bbb_sample_weights, K % 8 == 0) + elbo_finalize on a (8, 16) layer, S = 4, epsilon from ops.philox_normal."""
    K, N, S = 8, 16, 4
    pr = R.PRIORS[prior]
    t = Tally(f"k1s {prior}")
    ew, eb = _philox(S, N, K, dev)
    for c in R.cells(prior):
        p = R.cell_params(c, N, K)
        w_mu, w_rho, b_mu, b_rho = (_up(a, dev) for a in p)
        sm = ops.bbb_sample_weights([dict(w_mu=w_mu, w_rho=w_rho, b_mu=b_mu, b_rho=b_rho, prior=_spec(pr), layer_id=LAYER_ID)],
                                    n_samples=S, seed=SEED, sample_offset=OFFSET)[0]
        fin = ops.elbo_finalize(workspaces=[sm["workspace"]], layer_in=[K], layer_out=[N], local_reparam=False, prior=_spec(pr),
                                n_samples=S, logits=None, target=None, mode=None)
        ref = R.bbb_ref(np.zeros((1, K)), *p, ew, eb, pr)
        judge_rho(t, c, "log_q", fin["log_q"].cpu().numpy(), ref.log_q, ref.b_log_q)
        judge_log_prior(t, c, pr, fin["log_prior"].cpu().numpy(), ref.log_prior, ref.b_log_prior, ref.m)
        if c.rho != 89.0:                                            # the sampled bias is fp32: fma(sigma, eps, mu)
            db = np.abs(eb) * R.rel_sigma(p[3].astype(np.float64)) * R.softplus64(p[3]) + R.U * np.abs(ref.bias)
            t.add("b", R.share(sm["b"].cpu().numpy(), ref.bias, db), c.name)
    t.report()


@pytest.mark.parametrize("prior", list(R.PRIORS))
def test_flipout_prepare_statistics_cell_by_cell(dev, prior):
    K, N, D = 8, 16, 4
    pr = R.PRIORS[prior]
    t = Tally(f"flipout {prior}")
    ew, eb = R.cell_eps(D, N, K)
    dw, db = _dev_eps(D, N, K, dev)
    for c in R.cells(prior):
        p = R.cell_params(c, N, K)
        out = ops.flipout_prepare(*(_up(a, dev) for a in p), n_samples=D, n_draws=D, prior=_spec(pr), math_mode=L.MATH_F32,
                                  eps_mode=L.EPS_MEMORY, eps_w=dw, eps_b=db, want_stats=True, want_eps=True)
        assert torch.equal(out["eps_w"], dw) and torch.equal(out["eps_b"], db)
        ref = R.bbb_ref(np.zeros((1, K)), *p, ew, eb, pr)
        judge_rho(t, c, "log_q", out["log_q"].cpu().numpy(), ref.log_q, ref.b_log_q)
        judge_log_prior(t, c, pr, out["log_prior"].cpu().numpy(), ref.log_prior, ref.b_log_prior, ref.m)
    t.report()


@pytest.mark.parametrize("prior", list(R.PRIORS))
@pytest.mark.parametrize("keep", [0.5, 0.12])
def test_sparse_elbo_terms_cell_by_cell(dev, keep, prior):
    """A 16 x 8 layer with half and with an eighth of its weights kept (rows without a survivor among them), a third of the
    biases pruned; sigma_val as bnn_softplus leaves it; epsilon is the dense map's at the kept positions."""
    N, K, S = 16, 8, 4
    pr = R.PRIORS[prior]
    t = Tally(f"sparse keep {keep} {prior}")
    rs = np.random.RandomState(int(keep * 100))
    mask = rs.uniform(size=(N, K)) < keep
    bkeep = rs.uniform(size=N) < 0.67
    rows, cols = np.nonzero(mask)
    row_ptr = _up(np.concatenate([[0], np.cumsum(mask.sum(1))]).astype(np.int32), dev)
    col = _up(cols.astype(np.int16), dev)
    ew, eb = _philox(S, N, K, dev)
    eps = np.concatenate([ew[:, rows, cols], eb[:, bkeep]], 1)
    lp, lq = torch.empty(S, device=dev), torch.empty(S, device=dev)
    for c in R.cells(prior):
        w_mu, w_rho, b_mu, b_rho = R.cell_params(c, N, K)
        layer = dict(row_ptr=row_ptr, col=col, mu_val=_up(w_mu[mask], dev), sigma_val=ops.softplus(_up(w_rho[mask], dev)),
                     b_mu=_up(b_mu, dev), b_sigma=ops.softplus(_up(b_rho, dev)), b_keep=_up(bkeep.astype(np.uint8), dev),
                     in_features=K, out_features=N, nnz=int(mask.sum()), layer_id=LAYER_ID)
        a = ops.sparse_elbo_terms_args([layer], n_samples=S, prior=_spec(pr), log_prior=lp, log_q=lq,
                                       workspace=ops.sparse_elbo_terms_workspace([layer], S, dev), seed=SEED, sample_offset=OFFSET)
        ops.sparse_elbo_terms(a)
        ref = R.stats_ref(np.concatenate([w_mu[mask], b_mu[bkeep]]), np.concatenate([w_rho[mask], b_rho[bkeep]]), eps, pr)
        judge_rho(t, c, "log_q", lq.cpu().numpy(), ref.log_q, ref.b_log_q)
        judge_log_prior(t, c, pr, lp.cpu().numpy(), ref.log_prior, ref.b_log_prior, ref.m)
    t.report()


@pytest.mark.parametrize("prior", list(R.PRIORS))
def test_bbb_group_loss_info_cell_by_cell(dev, prior):
    """One agent, an 8-16-16-1 network, one minibatch at learning rate 0: loss_info's mean log p and mean log q over S = 4
    draws.  A mean is judged by the worst of its samples' regimes; the three layers are rounded to fp32 one by one before
    they are added (8 u of the total on top of the bound)."""
    I, H, S, B, first = 8, 16, 4, 4, 5
    pr = R.PRIORS[prior]
    t = Tally(f"bbb_group {prior}")
    dims = ((H, I), (H, H), (1, H))
    eps = np.concatenate([np.concatenate([a.reshape(S, -1), b.reshape(S, -1)], 1)
                          for a, b in (_philox(S, n, k, dev, seed=SEED, layer_id=li, first=first) for li, (n, k) in enumerate(dims))], 1)
    assert ops.bbb_group_workspace_bytes(I, H) > 0
    slab, targets = _up(R.cell_x(B, I, 1), dev), torch.zeros(B, device=dev)
    for c in R.cells(prior):
        ps = [R.cell_params(c, n, k) for n, k in dims]
        params = [_up(a, dev) for p in ps for a in p]
        loss = torch.zeros(4, device=dev)
        ag = ops.bbb_group_agent(params=params, exp_avg=[torch.zeros_like(p) for p in params], exp_avg_sq=[torch.zeros_like(p) for p in params],
                                 step=torch.zeros(1, dtype=torch.int32, device=dev), lr=torch.zeros(1, device=dev), slab=slab, targets=targets,
                                 n_batches=torch.ones(1, dtype=torch.int32, device=dev), loss_info=loss,
                                 sample_counter=torch.tensor([first], dtype=torch.int32, device=dev),
                                 workspace=torch.zeros(ops.bbb_group_workspace_bytes(I, H) // 4, device=dev), eps_seed=SEED)
        ops.bbb_group_train(ops.bbb_group_args([ag], in_features=I, hidden=H, n_samples=S, device=dev, prior=_spec(pr), batch=B,
                                               max_batches=1, kl_weights=[1.0]))
        got = loss.cpu().numpy().astype(np.float64)
        ref = R.stats_ref(np.concatenate([np.concatenate([p[0].ravel(), p[2]]) for p in ps]),
                          np.concatenate([np.concatenate([p[1].ravel(), p[3]]) for p in ps]), eps, pr)
        judge_rho(t, c, "mean log_q", got[2], ref.log_q.mean(), ref.b_log_q.mean() + 8 * R.U * abs(ref.log_q.mean()))
        if c.rho == 89.0:
            assert not np.isfinite(got[1]), (c.name, got)
            continue
        tags = R.prior_sample_tags(pr, ref.m)
        bound = ref.b_log_prior.mean() + 8 * R.U * abs(ref.log_prior.mean())
        if "beyond" in tags:
            assert not np.isfinite(got[1]), (c.name, got)
        elif "open" in tags:
            pass
        elif "band" in tags:
            assert (np.isinf(got[1]) and got[1] < 0) or abs(got[1] - ref.log_prior.mean()) <= bound, (c.name, got)
            if c.tag == "band":
                t.note("mean log_p", bool(np.isinf(got[1])))
        else:
            t.add("mean log_p", R.share(got[1], ref.log_prior.mean(), bound), c.name)
    t.report()


# ----------------------------------------------------------------------------------------------------------- the KL
KL_NAMES = ("kl", "ls", "s2", "m2")


def _judge_kl(t, c, got, ref, names=KL_NAMES):
    for name, g, v, b in zip(names, got, ref.value, ref.bound):
        if name == "m2" or (name == "s2" and c.rho != 89.0):      # no edge reaches sum mu^2; only sigma = +inf reaches sum sigma^2
            t.add(name, R.share(g, v, b), c.name)
        else:
            judge_rho(t, c, name, g, v, b)


@pytest.mark.parametrize("sp", list(R.LR_SIGMA_P))
@pytest.mark.parametrize("n", [1, 7, 1027])
def test_gauss_kl_cell_by_cell(dev, n, sp):
    t = Tally(f"gauss_kl n = {n} {sp}")
    for c in R.lr_cells(sp):
        mu, rho = R.cell_params(c, 1, n)[:2]
        got = ops.gauss_kl(_up(mu.ravel(), dev), _up(rho.ravel(), dev), R.LR_SIGMA_P[sp]).cpu().numpy()
        _judge_kl(t, c, got, R.kl_ref(mu, rho, R.LR_SIGMA_P[sp]))
    t.report()


def _lr_refs(p, sp):
    w_mu, w_rho, b_mu, b_rho = p
    allp = R.kl_ref(np.concatenate([w_mu.ravel(), b_mu]), np.concatenate([w_rho.ravel(), b_rho]), sp)
    return allp, R.kl_ref(w_mu, w_rho, sp), R.kl_ref(b_mu, b_rho, sp)


@pytest.mark.parametrize("sp", list(R.LR_SIGMA_P))
@pytest.mark.parametrize("form", ["tile", "gemm", "gemm-prepared"])
def test_lr_linear_fwd_fused_kl_cell_by_cell(dev, form, sp):
    """kl3 = (KL, weight KL, bias KL) of lr_linear_fwd(want_kl, want_scalars) at (8, 16, 16, 3): the tile form in fp32 math,
    the block form on bf16 x with and without lr_prepare's fragments (whose launch then owns the workspace sums)."""
    K, N, B, S = 8, 16, 16, 3
    spv = R.LR_SIGMA_P[sp]
    t = Tally(f"lr_linear_fwd {form} {sp}")
    x = _up(R.cell_x(B, K), dev)
    for i, c in enumerate(R.lr_cells(sp)):
        p = R.cell_params(c, N, K, lr=True)
        d = [_up(a, dev) for a in p]
        kw = dict(n_samples=S, sigma_p=spv, relu=False, y_dtype=torch.float32, eps_mode=L.EPS_PHILOX, seed=SEED, layer_id=LAYER_ID,
                  sample_offset=OFFSET, want_kl=True, want_scalars=True)
        if form == "tile":
            args, kw = (x,), dict(kw, math_mode=L.MATH_F32, form=L.FORM_TILE)
        else:
            x16 = x.to(torch.bfloat16)
            wfrag, ws = ops.lr_prepare(*d) if form == "gemm-prepared" else (None, None)
            args, kw = (x16,), dict(kw, math_mode=L.MATH_BF16, form=L.FORM_GEMM, x_sq=(x16 * x16), w_frag=wfrag, workspace=ws)
        if i == 0:
            assert ops.lr_plan(*args, *d, **kw)["form"] == (L.FORM_TILE if form == "tile" else L.FORM_GEMM)
        got = ops.lr_linear_fwd(*args, *d, **kw)["kl3"].cpu().numpy()
        allp, wp, bp = _lr_refs(p, spv)
        judge_rho(t, c, "kl", got[0], allp.value[0], allp.bound[0])
        judge_rho(t, c, "bias_kl", got[2], bp.value[0], bp.bound[0])
        judge_rho(t, c, "weight_kl", got[1], wp.value[0], allp.bound[0] + bp.bound[0], difference=True)     # kl - bias_kl
    t.report()


@pytest.mark.parametrize("sp", list(R.LR_SIGMA_P))
def test_lr_prepare_workspace_kl_cell_by_cell(dev, sp):
    """lr_prepare's KL sums, read the way an evaluation reads them: elbo_finalize(local_reparam) over the workspace."""
    K, N = 8, 16
    spv = R.LR_SIGMA_P[sp]
    t = Tally(f"lr_prepare {sp}")
    for c in R.lr_cells(sp):
        p = R.cell_params(c, N, K, lr=True)
        _, ws = ops.lr_prepare(*(_up(a, dev) for a in p))
        fin = ops.elbo_finalize(workspaces=[ws], layer_in=[K], layer_out=[N], local_reparam=True, prior=ops.PriorSpec(False, spv),
                                n_samples=1, logits=None, target=None, mode=None)
        allp = _lr_refs(p, spv)[0]
        judge_rho(t, c, "kl", fin["kl"].cpu().numpy(), allp.value[0], allp.bound[0])
    t.report()


def test_eval_prepare_sigma_cell_by_cell(dev):
    """eval_prepare's sigma = softplus(rho) of a (16, 8) tensor: within (E_SP + A_RHO |rho|) u of fp64 in every regular cell,
    +inf once exp overflows (rho > 88.72; the bound below it), exactly 0 at rho = -200, 0 or the denormal at rho = -100."""
    t = Tally("eval_prepare")
    for c in R.cells("gauss-1"):
        rho = R.cell_params(c, 16, 8)[1]
        got = ops.eval_prepare([_up(rho, dev)])[0][0].cpu().numpy().astype(np.float64)
        want = R.softplus64(rho)
        if c.rho == 89.0:                                        # the cell straddles exp's overflow at rho = 128 ln 2 = 88.72
            over = rho.astype(np.float64) > 88.73
            assert over.any() and np.all(np.isposinf(got[over])), c.name
            assert np.all(np.isposinf(got) | (np.abs(got - want) <= R.rel_sigma(rho.astype(np.float64)) * want)), c.name
        elif c.rho == -200.0:
            assert np.all(got == 0), c.name
        elif c.rho == R.RHO_BAND:
            assert np.all((got == 0) | (np.abs(got - want) <= 2.0 ** -149)), c.name
            t.note("sigma", bool(np.all(got == 0)))
        else:
            t.add("sigma", R.share(got, want, R.rel_sigma(rho.astype(np.float64)) * want), c.name)
    t.report()
