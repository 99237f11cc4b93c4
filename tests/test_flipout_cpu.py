"""CPU-side checks of the Flipout estimator (bnn_flipout_*, bnn_hip.flipout; include/bnn_hip.h F16; no GPU): the entry points
exist and the ABI version is unchanged, the ctypes mirrors match the header, every documented argument error fires on the host
in the documented order, the numpy restatement (tests/flipout_ref.py) equals the per-row dense definition and torch's CPU
autograd of it, the sign stream is balanced and uncorrelated, and BayesianNetwork.flipout() shares its Parameters."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import flipout_ref as R
from test_bandit_cpu import _layout

FAKE = 0x10000
NEW = ("bnn_flipout_signs", "bnn_flipout_prepare", "bnn_flipout_fwd", "bnn_flipout_bwd")
NULL, SHAPE, ENUM, WORKSPACE, ABI, ALIGN = -1, -2, -3, -4, -5, -6


def test_flipout_exports_and_abi_version():
    from bnn_hip import _lib as L
    lib = L.load()
    assert lib.bnn_version() == 9 == L.ABI_VERSION
    for name in NEW + ("bnn_flipout_prepare_workspace_bytes", "bnn_flipout_bwd_workspace_bytes"):
        assert name in L.EXPORTS and hasattr(lib, name)
    from bnn_hip import flipout, ops
    for name in ("flipout_signs", "flipout_prepare", "flipout_fwd", "flipout_bwd"):
        assert callable(getattr(ops, name))
    import networks
    assert networks.BayesianLinearFlipout is flipout.FlipoutLinear and networks.FlipoutNetwork is flipout.FlipoutNetwork
    assert callable(networks.BayesianNetwork.flipout)


def test_flipout_struct_layouts_match_the_header(tmp_path):
    from bnn_hip import _lib as L
    _layout(tmp_path, L.FlipoutSignsArgs, "bnn_flipout_signs_args",
            [("BNN_FLIPOUT_MAX_FEATURES", L.FLIPOUT_MAX_FEATURES), ("BNN_HIP_ABI_VERSION", L.ABI_VERSION), ("BNN_EPS_MAP_VERSION", 2)])
    _layout(tmp_path, L.FlipoutPrepareArgs, "bnn_flipout_prepare_args")
    _layout(tmp_path, L.FlipoutFwdArgs, "bnn_flipout_fwd_args")
    _layout(tmp_path, L.FlipoutBwdArgs, "bnn_flipout_bwd_args")


def _args(cls, ptrs, **over):
    a = cls()
    a.struct_bytes = C.sizeof(cls)
    for f in ptrs:
        setattr(a, f, FAKE)
    for k, v in over.items():
        if k.startswith("prior_"):
            setattr(a.prior, k[6:], v)
        else:
            setattr(a, k, v)
    return a


def _signs(**over):
    from bnn_hip import _lib as L
    return _args(L.FlipoutSignsArgs, ("out",), **dict(dict(n_samples=2, rows=3, cols=5, kind=0), **over))


PREP_PTRS = ("w_mu", "w_rho", "b_mu", "b_rho", "eps_w", "eps_b", "delta", "b_draw", "delta_bf16", "mu_bf16", "log_prior", "log_q",
             "eps_w_dump", "eps_b_dump", "workspace")


def _prep(**over):
    from bnn_hip import _lib as L
    d = dict(n_samples=4, n_draws=2, in_features=37, out_features=21, eps_mode=L.EPS_MEMORY, math=L.MATH_BF16, want_stats=1,
             prior_kind=L.PRIOR_GAUSS, prior_sigma_p=1.0, workspace_bytes=1 << 20)
    return _args(L.FlipoutPrepareArgs, PREP_PTRS, **dict(d, **over))


FWD_PTRS = ("x", "w_mu", "delta", "mu_bf16", "delta_bf16", "b_draw", "y")


def _fwd(**over):
    from bnn_hip import _lib as L
    d = dict(n_samples=4, n_draws=2, batch=19, in_features=37, out_features=21, x_dtype=L.F32, x_per_sample=0, math=L.MATH_F32,
             eps_mode=L.EPS_PHILOX, y_dtype=L.F32)
    return _args(L.FlipoutFwdArgs, FWD_PTRS, **dict(d, **over))


BWD_PTRS = ("x", "gy", "y", "w_mu", "w_rho", "b_mu", "b_rho", "eps_w", "eps_b", "g_log_prior", "g_log_q", "g_w_mu", "g_w_rho", "g_b_mu",
            "g_b_rho", "g_x", "workspace")


def _bwd(**over):
    from bnn_hip import _lib as L
    d = dict(n_samples=4, n_draws=2, batch=19, in_features=37, out_features=21, x_per_sample=0, relu=1, prior_kind=L.PRIOR_GAUSS,
             prior_sigma_p=1.0, workspace_bytes=1 << 24)
    return _args(L.FlipoutBwdArgs, BWD_PTRS, **dict(d, **over))


def _first(fn, make, size, cases):
    """Every case alone gives its status; a call broken in two ways gives the status of the EARLIER class."""
    assert fn(None, None) == NULL
    for delta in (8, -8):
        assert fn(C.byref(make(struct_bytes=size + delta)), None) == ABI
    flat = [(st, bad) for st, bads in cases for bad in bads]
    for st, bad in flat:
        assert fn(C.byref(make(**bad)), None) == st, bad
    for i, (st, bad) in enumerate(flat):                       # documented order: the first class in `cases` wins
        for st2, bad2 in flat[i + 1:]:
            if st2 != st and not (set(bad) & set(bad2)) and not all(k.startswith("prior_") for k in (*bad, *bad2)):
                assert fn(C.byref(make(**dict(bad, **bad2))), None) == st, (bad, bad2)
        assert fn(C.byref(make(struct_bytes=size + 8, **bad)), None) == ABI


def test_signs_argument_errors_in_the_documented_order():
    from bnn_hip import _lib as L
    _first(L.load().bnn_flipout_signs, _signs, C.sizeof(L.FlipoutSignsArgs),
           [(SHAPE, (dict(n_samples=0), dict(rows=0), dict(cols=-1))), (ENUM, (dict(kind=2), dict(kind=-1))), (NULL, (dict(out=None),))])


def test_prepare_argument_errors_in_the_documented_order():
    from bnn_hip import _lib as L
    lib = L.load()
    need = lib.bnn_flipout_prepare_workspace_bytes(2, 37, 21)
    assert need > 0 and lib.bnn_flipout_prepare_workspace_bytes(0, 37, 21) == 0 == lib.bnn_flipout_prepare_workspace_bytes(2, 0, 21)
    assert lib.bnn_flipout_prepare_workspace_bytes(2, L.FLIPOUT_MAX_FEATURES + 1, 21) == 0
    _first(lib.bnn_flipout_prepare, _prep, C.sizeof(L.FlipoutPrepareArgs), [
        (SHAPE, (dict(n_samples=0), dict(n_draws=0), dict(n_samples=5), dict(in_features=0), dict(out_features=L.FLIPOUT_MAX_FEATURES + 1),
                 dict(prior_sigma_p=0.0))),
        (ENUM, (dict(eps_mode=3), dict(math=L.MATH_BF16X3), dict(math=7), dict(prior_kind=2))),
        (NULL, tuple({f: None} for f in ("w_mu", "w_rho", "b_mu", "b_rho", "delta", "b_draw", "eps_w", "eps_b", "delta_bf16", "mu_bf16",
                                         "log_prior", "log_q"))),
        (WORKSPACE, (dict(workspace=None), dict(workspace_bytes=need - 1))),
        (ALIGN, (dict(w_mu=FAKE + 2), dict(delta=FAKE + 1), dict(eps_w_dump=FAKE + 2), dict(mu_bf16=FAKE + 1), dict(workspace=FAKE + 4))),
    ])
    fn = lib.bnn_flipout_prepare
    # what a mode does not read may be absent
    assert fn(C.byref(_prep(eps_mode=L.EPS_PHILOX, eps_w=None, eps_b=None, math=L.MATH_F32, delta_bf16=None, mu_bf16=None,
                            want_stats=0, log_prior=None, log_q=None, workspace=None, prior_sigma_p=0.0, n_samples=0)), None) == SHAPE
    assert fn(C.byref(_prep(prior_kind=L.PRIOR_MIXTURE, prior_sigma1=0.0, prior_sigma2=1.0)), None) == SHAPE


def test_fwd_argument_errors_in_the_documented_order():
    from bnn_hip import _lib as L
    lib = L.load()
    _first(lib.bnn_flipout_fwd, _fwd, C.sizeof(L.FlipoutFwdArgs), [
        (SHAPE, (dict(n_samples=0), dict(n_draws=0), dict(n_draws=3), dict(batch=0), dict(in_features=0), dict(out_features=0),
                 dict(in_features=L.FLIPOUT_MAX_FEATURES + 1), dict(x_per_sample=2))),
        (ENUM, (dict(math=L.MATH_BF16X3), dict(eps_mode=3), dict(x_dtype=2), dict(y_dtype=L.BF16), dict(x_dtype=L.BF16))),
        (NULL, (dict(x=None), dict(y=None), dict(b_draw=None), dict(w_mu=None), dict(delta=None))),
        (ALIGN, (dict(x=FAKE + 2), dict(y=FAKE + 2), dict(b_draw=FAKE + 1), dict(w_mu=FAKE + 2), dict(delta=FAKE + 2))),
    ])
    fn = lib.bnn_flipout_fwd
    assert fn(C.byref(_fwd(eps_mode=L.EPS_ZERO)), None) == SHAPE                       # the mean path is one "sample"
    bf = dict(math=L.MATH_BF16, x_dtype=L.BF16, y_dtype=L.BF16, w_mu=None, delta=None)
    assert fn(C.byref(_fwd(mu_bf16=None, **bf)), None) == NULL and fn(C.byref(_fwd(delta_bf16=None, **bf)), None) == NULL
    assert fn(C.byref(_fwd(x=FAKE + 1, **bf)), None) == ALIGN and fn(C.byref(_fwd(mu_bf16=FAKE + 1, **bf)), None) == ALIGN


def test_bwd_argument_errors_in_the_documented_order():
    from bnn_hip import _lib as L
    lib = L.load()
    need = lib.bnn_flipout_bwd_workspace_bytes(4, 19, 37, 21)
    assert need == 4 * 19 * (2 * 21 + 37) * 4 and lib.bnn_flipout_bwd_workspace_bytes(0, 19, 37, 21) == 0
    _first(lib.bnn_flipout_bwd, _bwd, C.sizeof(L.FlipoutBwdArgs), [
        (SHAPE, (dict(n_samples=0), dict(n_draws=0), dict(n_draws=3), dict(batch=0), dict(in_features=0), dict(out_features=0),
                 dict(x_per_sample=-1), dict(prior_sigma_p=-1.0))),
        (ENUM, (dict(prior_kind=2),)),
        (NULL, tuple({f: None} for f in ("x", "gy", "y", "w_mu", "w_rho", "b_mu", "b_rho", "eps_w", "eps_b", "g_w_mu", "g_w_rho", "g_b_mu",
                                         "g_b_rho"))),
        (WORKSPACE, (dict(workspace=None), dict(workspace_bytes=need - 1))),
        (ALIGN, (dict(x=FAKE + 2), dict(g_x=FAKE + 2), dict(g_log_q=FAKE + 1), dict(workspace=FAKE + 2))),
    ])
    # optional pointers may be absent (a fake stream is never reached: the launch itself is not made without a device)
    assert lib.bnn_flipout_bwd(C.byref(_bwd(relu=0, y=None, workspace=None)), None) == WORKSPACE


# ---------------------------------------------------------------------------------------------- the restatement itself
def _layer_case(seed, B, K, N, S, D, per_sample):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((S, B, K) if per_sample else (B, K))
    mu, rho = rng.uniform(-0.3, 0.3, (N, K)), rng.uniform(-3.0, -1.0, (N, K))
    bm, br = rng.uniform(-0.3, 0.3, N), rng.uniform(-3.0, -1.0, N)
    ew, eb = rng.standard_normal((D, N, K)), rng.standard_normal((D, N))
    r = R.sign_block(2026, 1, 0, 5, S, B, K).astype(np.float64)
    s = R.sign_block(2026, 1, 1, 5, S, B, N).astype(np.float64)
    return x, mu, rho, bm, br, ew, eb, r, s


@pytest.mark.parametrize("B,K,N,S,D,per_sample", [(5, 7, 3, 4, 2, False), (3, 130, 4, 6, 3, True), (1, 1, 1, 2, 1, False), (4, 9, 6, 3, 3, True)])
def test_restated_forward_is_the_per_row_dense_form(B, K, N, S, D, per_sample):
    x, mu, rho, bm, br, ew, eb, r, s = _layer_case(11, B, K, N, S, D, per_sample)
    delta = R.softplus(rho) * ew
    b = bm + R.softplus(br) * eb
    for relu in (False, True):
        y, _ = R.forward(x, mu, delta, b, r, s, relu)
        want = R.forward_dense(x, mu, delta, b, r, s, relu)
        scale = np.abs(want).max()
        assert np.abs(y - want).max() <= 1e-12 * scale


@pytest.mark.parametrize("prior", [("gauss", 0.7), ("mixture", 0.5, 1.0, math.exp(-3.0))])
@pytest.mark.parametrize("B,K,N,S,D,per_sample,relu", [(5, 7, 3, 4, 2, False, True), (3, 9, 4, 6, 3, True, False), (2, 4, 2, 2, 1, True, True)])
def test_restated_gradients_equal_autograd_of_the_dense_form(prior, B, K, N, S, D, per_sample, relu):
    x, mu, rho, bm, br, ew, eb, r, s = _layer_case(23, B, K, N, S, D, per_sample)
    rng = np.random.default_rng(5)
    gy, glp, glq = rng.standard_normal((S, B, N)), rng.standard_normal(D), rng.standard_normal(D)
    T = lambda a, g=False: torch.tensor(a, dtype=torch.float64, requires_grad=g)
    tx, tmu, trho, tbm, tbr = T(x, True), T(mu, True), T(rho, True), T(bm, True), T(br, True)
    sw, sb = torch.log1p(torch.exp(trho)), torch.log1p(torch.exp(tbr))
    xs = tx if per_sample else tx.unsqueeze(0).expand(S, B, K)
    ys = []
    for i in range(S):
        d = i // (S // D)
        w = tmu.unsqueeze(0) + (sw * T(ew[d])).unsqueeze(0) * (T(s[i]).unsqueeze(2) * T(r[i]).unsqueeze(1))       # [B, N, K]
        ys.append(torch.einsum("bnk,bk->bn", w, xs[i]) + tbm + sb * T(eb[d]))
    y = torch.stack(ys)
    if relu:
        y = torch.relu(y)
    loss = (T(gy) * y).sum()

    def ln(w, sd):
        return R.C0 - math.log(sd) - w ** 2 / (2.0 * sd * sd)
    for d in range(D):
        w, b = tmu + sw * T(ew[d]), tbm + sb * T(eb[d])
        if prior[0] == "gauss":
            lp = ln(w, prior[1]).sum() + ln(b, prior[1]).sum()
        else:
            f = lambda t: torch.log(prior[1] * torch.exp(ln(t, prior[2])) + (1 - prior[1]) * torch.exp(ln(t, prior[3]))).sum()
            lp = f(w) + f(b)
        lq = (R.C0 - torch.log(sw) - (w - tmu) ** 2 / (2 * sw ** 2)).sum() + (R.C0 - torch.log(sb) - (b - tbm) ** 2 / (2 * sb ** 2)).sum()
        loss = loss + glp[d] * lp + glq[d] * lq
    loss.backward()
    got = R.backward(x, gy, y.detach().numpy(), mu, rho, bm, br, ew, eb, r, s, prior, relu, glp, glq)
    gx = got[4] if per_sample else got[4].sum(0)
    for g, t in zip(got[:4] + (gx,), (tmu, trho, tbm, tbr, tx)):
        np.testing.assert_allclose(g, t.grad.numpy(), rtol=1e-9, atol=1e-12 * np.abs(t.grad.numpy()).max())
    # the ELBO terms the loss used are the restatement's
    lp_ref, lq_ref = R.elbo_terms(mu, rho, bm, br, ew, eb, prior)
    w0, b0 = mu + R.softplus(rho) * ew[0], bm + R.softplus(br) * eb[0]
    assert abs(lp_ref[0] - R.log_prior(w0, b0, prior)) <= 1e-12 * abs(lp_ref[0])


def test_sign_stream_balance_and_independence():
    """seed 2026, layers 0-2, [64, 300], samples 5 and 6: six sums of +-1 products, each / sqrt(n) within 4."""
    rows, cols = 64, 300
    for layer in range(3):
        r5, r6 = (R.signs(2026, layer, 0, g, rows, cols).astype(np.int64) for g in (5, 6))
        s5 = R.signs(2026, layer, 1, 5, rows, cols).astype(np.int64)
        assert set(np.unique(r5)) == {-1, 1}
        stats = {
            "sum r": (r5.sum(), r5.size), "sum s": (s5.sum(), s5.size), "r.s": ((r5 * s5).sum(), r5.size),
            "r(5).r(6)": ((r5 * r6).sum(), r5.size),
            "rows": ((r5[1:] * r5[:-1]).sum(), r5[1:].size), "cols": ((r5[:, 1:] * r5[:, :-1]).sum(), r5[:, 1:].size),
        }
        for name, (v, n) in stats.items():
            assert abs(v) / math.sqrt(n) <= 4.0, (layer, name, v / math.sqrt(n))


def test_signs_do_not_depend_on_how_a_batch_is_cut():
    whole = R.signs(7, 2, 1, 3, 19, 130)
    parts = np.concatenate([R.signs(7, 2, 1, 3, 7, 130), R.signs(7, 2, 1, 3, 12, 130, row_offset=7)])
    assert (whole == parts).all()
    assert (R.signs(7, 2, 1, 3, 19, 130) != R.signs(7, 2, 0, 3, 19, 130)).any()            # r and s are different streams


# ---------------------------------------------------------------------------------------------- host surface
MP = dict(input_shape=37, classes=5, batch_size=19, hidden_units=21, mode="classification", mu_init=[-0.2, 0.2], rho_init=[-5, -4],
          prior_init=[0.5, 0, -6], mixture_prior=True, local_reparam=False)


def test_flipout_view_shares_the_parameters():
    import networks
    net = networks.BayesianNetwork(MP)
    f = net.flipout(base_draws=2)
    assert isinstance(f, networks.FlipoutNetwork) and f.base_draws == 2
    assert list(f.state_dict().keys()) == list(net.state_dict().keys())
    for (ka, a), (kb, b) in zip(net.named_parameters(), f.named_parameters()):
        assert ka == kb and a is b and a.data_ptr() == b.data_ptr()
    own = networks.FlipoutNetwork(MP)
    assert list(own.state_dict().keys()) == list(net.state_dict().keys())
    own.load_state_dict(net.state_dict())                                  # state dicts interchange
    lin = networks.BayesianLinearFlipout(7, 3, [-0.2, 0.2], [-5, -4], [0.5, 0, -6])
    ref = networks.BayesianLinear(7, 3, [-0.2, 0.2], [-5, -4], [0.5, 0, -6])
    assert {k: tuple(v.shape) for k, v in lin.state_dict().items()} == {k: tuple(v.shape) for k, v in ref.state_dict().items()}


def test_host_side_refusals():
    import networks
    from bnn_hip import active
    from bnn_hip.ops import BnnHipError
    with pytest.raises(BnnHipError, match="local_reparam"):
        networks.FlipoutNetwork(dict(MP, local_reparam=True, mixture_prior=False, prior_init=[1.0]))
    with pytest.raises(BnnHipError, match="local_reparam"):
        networks.BayesianNetwork(dict(MP, local_reparam=True, mixture_prior=False, prior_init=[1.0])).flipout()
    f = networks.BayesianNetwork(MP).flipout()
    with pytest.raises(BnnHipError, match="per row"):
        active.check_joint(f)
    with pytest.raises(BnnHipError, match="divide"):
        f._draws(6, 4)
    with pytest.raises(BnnHipError, match="stacked"):
        f.predictive(torch.zeros(19, 37), 4, stacked=True)
    with pytest.raises(BnnHipError, match="stacked"):
        f.score(torch.zeros(19, 37), torch.zeros(19, dtype=torch.long), 4, stacked=True)
    with pytest.raises(BnnHipError):
        f.forward_mc(torch.zeros(19, 37), 4)                                # CPU tensors: no fallback
