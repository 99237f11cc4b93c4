"""The ELBO loss tail -- logits -> per-sample NLL, ELBO sums, training loss and logit gradient -- against float64
(tests/loss_tail_ref.py) on every form that computes it: K4 (elbo_finalize_kernel, bnn_fin.h fin_nll) in its three launch
modes and every class-count branch, nll_rows_kernel, the fused last-layer forms K1c / K1r / K3r with their inline NLL and
fin_loss_row_grad / fin_loss_assemble, elbo_loss_nll_bwd_kernel and nll_bwd_kernel.  Where a layer produced the logits,
the reference is built from the launch's own logits (res["y"]) and per-sample scalars, so the bound covers only the
tail's fp32 rounding.  Labels -1 and C poison exactly their rows (NaN), never anything else.

Which form a fused-final case took is read off the scratch: it is filled with NaN past its ticket words before the call;
the row-split forms K1r / K3r (and K1c when it splits K into slices) write their per-sample partials there, the two-launch
fallback does not touch it (N <= 16: nll_rows_kernel is not entered)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bnn_hip
import loss_tail_ref as R
from bnn_hip import _lib as L
from bnn_hip import ops, synth
from oracle import bnn_oracle as O

SIGMA = 0.7
NAN_BITS = 0x7FC00000


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _f32_math():
    bnn_hip.set_math("f32")
    yield
    bnn_hip.set_math("bf16")


def np64(t):
    return t.detach().double().cpu().numpy()


def inputs(mode, S, B, C, seed, groups=1):
    lg = R.make_logits(S, B, C, seed, special=mode == "classification")
    tg = R.make_labels(B, C, seed, groups) if mode == "classification" else R.make_reg_targets(B, C, seed, groups)
    return lg, tg


def dev_target(tg, dev, offset=False):
    """The device target: [B] / [B, C] for one block (tg[0]), [G, ...] per group; `offset`: 4 bytes past a 16-byte
    boundary (a regression target that cannot take the float4 loads)."""
    t = tg[0] if tg.shape[0] == 1 else tg
    if not offset:
        return torch.from_numpy(np.ascontiguousarray(t)).to(dev)
    buf = torch.zeros(t.size + 4, dtype=torch.float32, device=dev)
    view = buf[1:1 + t.size].view(t.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(t)))
    assert view.data_ptr() % 16 == 4
    return view


def sentinel_scratch(S, dev):
    """ops.final_scratch with every word past the per-sample tickets set to NaN."""
    sc = ops.final_scratch(S, dev)
    sc[(S * 4 + 255) // 256 * 64:] = NAN_BITS
    return sc


def scratch_written(sc, S, lo_bytes, n_floats):
    f = sc.view(torch.float32)
    lo = (S * 4 + 255) // 256 * 64 + lo_bytes // 4
    return bool(torch.isfinite(f[lo:lo + n_floats]).any())


def tickets_zero(sc, S):
    return int(sc[:S].abs().sum()) == 0


def check_nll(got, lg, tg, mode, what):
    R.assert_close(np64(got), R.nll(lg, tg, mode, SIGMA), R.nll_tol(lg, tg, mode, SIGMA), what)


def check_sums(sums, nll_got, group, what):
    """sums[:, 2] against the fp64 fold of the launch's own per-sample nll, sums[:, 3] == group size exactly."""
    n = np64(nll_got)
    want = R.elbo_sums(None, None, n, group)
    s = np64(sums)
    R.assert_close(s[:, 2], want[:, 2], R.ULP * np.abs(want[:, 2]) + 1e-30, what + " sums")    # an fp64 fold, rounded once
    assert (s[:, 3] == group).all(), what


# ------------------------------------------------------------------------------------------------------ 1. K4 sweep
# (mode, C, B, S, ticket, target offset): every fin_nll branch; across the list B covers {1, 17, 128, 300} and S the three
# launch modes of bnn_elbo_finalize -- one block (S = 1, or S <= 16 with S B C <= 65536 and no ticket), a block per sample
# folded by the ticket (1 < S <= 64 with a ticket), a block per sample + sample_sums_kernel (S = 65, or no ticket and
# S B C > 65536)
K4_CASES = [
    ("classification", 1, 17, 1, False, False),      # C <= 16 global form, clamped loads; single
    ("classification", 2, 300, 17, True, False),     # ticket
    ("classification", 3, 128, 65, False, False),    # follow-up
    ("classification", 10, 1, 4, False, False),      # single (small)
    ("classification", 15, 300, 64, True, False),    # ticket
    ("classification", 16, 17, 65, True, False),     # ldc == 16 && C <= 16 tile form; follow-up (ticket ignored past 64)
    ("classification", 17, 128, 2, False, False),    # C <= 32 rolled loop; single
    ("classification", 31, 300, 17, True, False),
    ("classification", 32, 1, 65, False, False),
    ("classification", 33, 128, 4, False, False),    # C > 32 wave per row; single
    ("classification", 63, 17, 64, True, False),
    ("classification", 64, 300, 8, False, False),    # S B C > 65536, no ticket: follow-up
    ("classification", 65, 128, 1, False, False),
    ("classification", 100, 300, 17, True, False),
    ("classification", 1000, 17, 65, False, False),
    ("regression", 1, 300, 17, True, False),         # C <= 8 thread per row
    ("regression", 2, 128, 65, False, False),
    ("regression", 8, 17, 1, False, False),
    ("regression", 9, 300, 4, True, False),          # wide form, scalar loads (C % 4 != 0)
    ("regression", 16, 1, 64, True, False),          # wide form, float4 loads
    ("regression", 64, 128, 8, False, False),
    ("regression", 64, 17, 3, False, True),          # float4-shaped but the target is 4 bytes off: scalar branch
    ("regression", 65, 17, 17, True, False),
    ("regression", 4096, 17, 2, False, False),       # float4, many columns per lane
    ("regression", 4096, 1, 2, True, True),          # the same, scalar branch
]


def k4_id(case):
    """Test id naming the fin_nll branch and the launch mode of bnn_elbo_finalize a K4 case takes."""
    mode, C, B, S, ticketed, offset = case
    if mode == "classification":
        branch = "tile16" if C == 16 else "clamped16" if C < 16 else "rolled32" if C <= 32 else "wave"
    else:
        branch = "thread" if C <= 8 else "wide_scalar" if (offset or C % 4) else "wide_float4"
    tk = ticketed and 1 < S <= 64
    launch = "single" if (S == 1 or (S <= 16 and S * B * C <= 65536 and not tk)) else "ticket" if tk else "followup"
    return f"{mode[:3]}-C{C}-B{B}-S{S}-{branch}-{launch}"


def k4_call(dev, lg_t, tgt, mode, S, **kw):
    return ops.elbo_finalize(workspaces=[], layer_in=[], layer_out=[], local_reparam=False, prior=ops.PriorSpec(),
                             n_samples=S, logits=lg_t, target=tgt, mode=mode, nll_sigma=SIGMA, **kw)


@pytest.mark.parametrize("mode,C,B,S,ticketed,offset", K4_CASES, ids=[k4_id(c) for c in K4_CASES])
def test_k4_finalize_against_fp64(dev, mode, C, B, S, ticketed, offset):
    lg, tg = inputs(mode, S, B, C, 100 + C)
    lg_t = torch.from_numpy(lg).to(dev)
    tgt = dev_target(tg, dev, offset)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    ticket = torch.zeros(1, dtype=torch.int32, device=dev) if ticketed else None
    sums = torch.full((1, 4), float("nan"), device=dev)
    first = None
    for launch in (1, 2):                                   # the second launch reuses the ticket word
        out = k4_call(dev, lg_t, tgt, mode, S, sample_counter=counter, sample_counter_inc=3 * S, sums=sums, ticket=ticket)
        torch.cuda.synchronize()
        check_nll(out["nll"], lg, tg, mode, f"launch {launch} nll")
        check_sums(sums, out["nll"], S, f"launch {launch}")
        assert (np64(sums)[:, :2] == 0).all()               # no layers: no complexity terms
        assert int(counter.item()) == 3 * S * launch        # advanced by inc, exactly once per launch
        assert ticket is None or int(ticket.item()) == 0
        if first is None:
            first = (out["nll"].clone(), sums.clone())
        else:                                               # deterministic: sample-order folds
            assert torch.equal(first[0], out["nll"]) and torch.equal(first[1], sums)


# ------------------------------------------------------------------------------------------------------ 2. nll_rows_kernel
@pytest.mark.parametrize("mode,C,B,S,enters", [("classification", 257, 128, 3, True), ("classification", 1000, 33, 2, True),
                                               ("regression", 4096, 17, 2, True), ("classification", 33, 65540, 1, False)],
                         ids=["cls-C257-B128-nll_rows", "cls-C1000-B33-nll_rows", "reg-C4096-B17-nll_rows", "cls-C33-B65540-past_16384_blocks"])
def test_nll_rows_kernel_against_fp64(dev, mode, C, B, S, enters):
    """C > 32 and B C >= 32768 with a scratch: the rows' NLL first, spread over row blocks (4 rows each); past 16384 row
    blocks per sample (B > 65536) the scratch has no room and the finalize walks the rows itself."""
    lg, tg = inputs(mode, S, B, C, 200 + C)
    lg_t, tgt = torch.from_numpy(lg).to(dev), dev_target(tg, dev)
    sc = sentinel_scratch(S, dev)
    with_rows = k4_call(dev, lg_t, tgt, mode, S, scratch=sc)["nll"]
    without = k4_call(dev, lg_t, tgt, mode, S)["nll"]
    torch.cuda.synchronize()
    assert scratch_written(sc, S, S * 8 * 16, S * ((B + 3) // 4)) == enters
    check_nll(with_rows, lg, tg, mode, "with scratch")
    check_nll(without, lg, tg, mode, "without scratch")


# ------------------------------------------------------------------------------------------------------ 3. per-group targets
@pytest.mark.parametrize("mode,C", [("classification", 10), ("classification", 16), ("classification", 17),
                                    ("classification", 33), ("classification", 100), ("regression", 1), ("regression", 65)])
@pytest.mark.parametrize("G,g,ticketed", [(3, 2, False), (4, 4, True), (5, 13, False)])   # one block / ticket / follow-up
def test_per_group_targets_against_fp64(dev, mode, C, G, g, ticketed):
    S, B = G * g, 37
    lg, tg = inputs(mode, S, B, C, 300 + C, groups=G)
    lg_t, tgt = torch.from_numpy(lg).to(dev), dev_target(tg, dev)
    sums = torch.full((G, 4), float("nan"), device=dev)
    ticket = torch.zeros(1, dtype=torch.int32, device=dev) if ticketed else None
    out = k4_call(dev, lg_t, tgt, mode, S, group_samples=g, sums=sums, ticket=ticket)
    torch.cuda.synchronize()
    check_nll(out["nll"], lg, tg, mode, "per-group nll")          # R.nll reads block s // g for sample s
    check_sums(sums, out["nll"], g, "per-group")
    # and not the first group's target for everyone
    wrong = R.nll(lg, tg[:1], mode, SIGMA)
    assert (np.abs(np64(out["nll"]) - wrong)[g:] > R.nll_tol(lg, tg, mode, SIGMA)[g:]).any()


# ------------------------------------------------------------------------------------------------------ 4./5. fused final forms
def layer_params(N, K, lr, seed):
    rs = np.random.RandomState(seed)
    shape = (K, N) if lr else (N, K)
    f = lambda *s: torch.from_numpy(rs.uniform(-0.2, 0.2, s).astype(np.float32))
    return (f(*shape), torch.from_numpy(rs.uniform(-5, -4, shape).astype(np.float32)), f(N),
            torch.from_numpy(rs.uniform(-5, -4, N).astype(np.float32)))


def run_final(dev, form, S, B, N, K, mode, tg, ticketed, loss=None, counter=None, seed=0, scratch=None, ticket=None):
    """One bbb_final_fwd / lr_final_fwd call.  form: "k1c" (the layer samples its weights), "k1r" (over bbb_sample_weights'
    draw), "k3r" (LR, the block parks the layer), "k3r_prep" (LR over lr_prepare's fragments).  `scratch` / `ticket`: the
    ones an earlier call left, instead of fresh ones.
    Returns (layer result, finalize result, sums, scratch, ticket)."""
    lr = form.startswith("k3r")
    p = [t.to(dev) for t in layer_params(N, K, lr, seed)]
    rs = np.random.RandomState(seed + 1)
    x = torch.from_numpy(rs.uniform(-1, 1, (B, K)).astype(np.float32)).to(dev)
    sc = sentinel_scratch(S, dev) if scratch is None else scratch
    if ticket is None and ticketed:
        ticket = torch.zeros(1, dtype=torch.int32, device=dev)
    prior = ops.PriorSpec()
    fin = dict(layer_in=[K], layer_out=[N], prior=prior, n_samples=S, target=dev_target(tg, dev), mode=mode, nll_sigma=SIGMA,
               scratch=sc, ticket=ticket, sums=torch.full((1, 4), float("nan"), device=dev), sample_counter=counter,
               sample_counter_inc=S if counter is not None else 0, loss=loss)
    if form == "k1c":
        res, out = ops.bbb_final_fwd((x,) + tuple(p), dict(n_samples=S, prior=prior, math_mode=L.MATH_F32, relu=False,
                                                            y_dtype=torch.float32, eps_mode=L.EPS_PHILOX, seed=11, layer_id=2,
                                                            want_stats=True), dict(workspaces=[], local_reparam=False, **fin))
    elif form == "k1r":
        sm = ops.bbb_sample_weights([dict(w_mu=p[0], w_rho=p[1], b_mu=p[2], b_rho=p[3], prior=prior, layer_id=2)],
                                    n_samples=S, seed=11)[0]
        res, out = ops.bbb_final_fwd((x.to(torch.bfloat16), None, None, None, None),
                                     dict(n_samples=S, prior=prior, math_mode=L.MATH_BF16, relu=False, y_dtype=torch.float32,
                                          eps_mode=L.EPS_ZERO, want_stats=False, w_sampled=sm["w"], b_sampled=sm["b"]),
                                     dict(workspaces=[sm["workspace"]], local_reparam=False, **fin))
    else:
        wfrag, ws = ops.lr_prepare(*p) if form == "k3r_prep" else (None, ops.lr_workspace(N, dev))
        res, out = ops.lr_final_fwd((x.to(torch.bfloat16),) + tuple(p),
                                    dict(w_frag=wfrag, workspace=ws, n_samples=S, sigma_p=prior.sigma_p, math_mode=L.MATH_BF16,
                                         relu=False, y_dtype=torch.float32, eps_mode=L.EPS_PHILOX, seed=11, layer_id=2,
                                         want_kl=True),
                                    dict(workspaces=[ws], local_reparam=True, **fin))
    torch.cuda.synchronize()
    return res, out, fin["sums"], sc, ticket


def expect_split(form, S, B, N, ticketed, loss):
    """The host's choice (bnn_bbb_final_fwd / bnn_lr_final_fwd): the row-split form (K1c: the one-launch form) or the
    two launches.  None: taken but not visible in the scratch (K1c with one K slice)."""
    if N > 16 or B > 128:
        return False
    if form == "k1c":
        return (S == 1 or S > 16 or ticketed) if S * 2 <= 128 else None
    if form == "k3r" and S > 16:
        return False
    return S == 1 or ticketed or (S > 64 and not loss)


def check_form(form, sc, S, B, N, ticketed, loss):
    want = expect_split(form, S, B, N, ticketed, loss)
    if want is not None:
        assert scratch_written(sc, S, 0, S * 16) == want, f"{form}: expected the {'split' if want else 'two-launch'} form"
    assert tickets_zero(sc, S)


FUSED = [  # (form, S, B, N): N over {1, 2, 3, 4, 5, 8, 10, 12, 15, 16} (float4 / scalar y stores), B over {1, 15, 16, 17, 127, 128}
    ("k1c", 1, 1, 1), ("k1c", 4, 15, 10), ("k1c", 16, 128, 16), ("k1c", 17, 17, 3), ("k1c", 40, 127, 8),
    ("k1r", 1, 16, 4), ("k1r", 2, 17, 5), ("k1r", 64, 128, 12), ("k1r", 65, 1, 15), ("k1r", 300, 127, 2),
    ("k3r", 1, 128, 10), ("k3r", 3, 17, 16), ("k3r", 16, 15, 1), ("k3r_prep", 2, 1, 8), ("k3r_prep", 65, 16, 3),
    ("k3r_prep", 300, 128, 4),
    ("k1c", 3, 129, 10), ("k1r", 3, 17, 17), ("k3r", 3, 129, 4), ("k3r_prep", 3, 16, 17),     # fallbacks
]


def fused_id(case):
    form, S, B, N = case
    taken = expect_split(form, S, B, N, True, False)
    return f"{form}-S{S}-B{B}-N{N}-{'y_float4' if N % 4 == 0 else 'y_scalar'}-{'two_launch' if taken is False else 'one_launch'}"


@pytest.mark.parametrize("form,S,B,N", FUSED, ids=[fused_id(c) for c in FUSED])
@pytest.mark.parametrize("mode", ["classification", "regression"])
def test_fused_final_forms_nll_against_fp64(dev, form, S, B, N, mode):
    K = 512 if form == "k1c" else 96                   # (K1c: two K slices, so that its form shows in the scratch)
    tg = R.make_labels(B, N, 400 + N) if mode == "classification" else R.make_reg_targets(B, N, 400 + N)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    res, out, sums, sc, ticket = run_final(dev, form, S, B, N, K, mode, tg, True, counter=counter, seed=N)
    lg = res["y"].cpu().numpy()
    check_nll(out["nll"], lg, tg, mode, form)
    check_sums(sums, out["nll"], S, form)
    assert int(counter.item()) == S and int(ticket.item()) == 0
    check_form(form, sc, S, B, N, True, False)


RELAUNCH = [  # (form, S, B, N)
    ("k1c", 4, 17, 10),           # K-slice tickets + the sample ticket
    ("k1r", 3, 17, 5),
    ("k3r", 2, 17, 16),           # parked
    ("k3r_prep", 64, 128, 4),     # 64 x 9 = 576 > 512 blocks: two tiles per row block, still ticketed
    ("k3r_prep", 65, 128, 4),     # no sample ticket: the follow-up sums launch
    ("k4", 10, 17, 17),           # bnn_elbo_finalize, a block per sample folded by the ticket
]


@pytest.mark.parametrize("form,S,B,N", RELAUNCH, ids=[f"{c[0]}-S{c[1]}-B{c[2]}-N{c[3]}" for c in RELAUNCH])
def test_second_launch_on_a_used_scratch_and_ticket(dev, form, S, B, N):
    """The hand-offs (bnn_fin.h fin_rows_meet / fin_samples_meet, K1c's K-slice stage) leave every ticket word at zero: a
    second call on the same scratch and ticket, same seed and no sample counter (so epsilon repeats), gives the same bits."""
    mode = "classification"
    tg = R.make_labels(B, N, 900 + N)
    sc, ticket, first = None, None, None
    if form == "k4":
        lg, _ = inputs(mode, S, B, N, 900 + N)
        lg_t, tgt = torch.from_numpy(lg).to(dev), dev_target(tg, dev)
        ticket = torch.zeros(1, dtype=torch.int32, device=dev)
    for launch in (1, 2):
        if form == "k4":
            sums = torch.full((1, 4), float("nan"), device=dev)
            out = k4_call(dev, lg_t, tgt, mode, S, sums=sums, ticket=ticket)
            torch.cuda.synchronize()
            got = [lg_t, out["nll"], sums]
        else:
            res, out, sums, sc, ticket = run_final(dev, form, S, B, N, 512 if form == "k1c" else 96, mode, tg, True, seed=N,
                                                   scratch=sc, ticket=ticket)
            got = [res["y"], out["nll"], sums] + ([out["kl"]] if form.startswith("k3r") else [out["log_prior"], out["log_q"]])
            assert tickets_zero(sc, S), f"launch {launch}"
        assert int(ticket.item()) == 0, f"launch {launch}"
        if first is None:
            first = [t.clone() for t in got]
        else:
            assert all(torch.equal(a, b) for a, b in zip(first, got))


LOSS_SHAPES = [(1, True), (2, True), (16, True), (64, True), (65, True), (128, True), (65, False), (128, False)]


@pytest.mark.parametrize("S,ticketed", LOSS_SHAPES)
@pytest.mark.parametrize("form", ["k1c", "k1r", "k3r_prep"])
def test_training_tail_against_fp64(dev, form, S, ticketed):
    """fin_kw["loss"]: out4, the seeds and the logit gradient against fp64 from the launch's own per-sample scalars and
    logits, at three betas.  ticket=None with S in {65, 128} took the row-split form and left out4 / g_a / g_b / g_kl3
    unwritten and the counter unadvanced; it now takes the two launches + the loss-tail launch."""
    B, N, K, mode = 37, 10, 512 if form == "k1c" else 96, "classification"
    tg = R.make_labels(B, N, 500 + S)
    lr = form.startswith("k3r")
    for bi, beta in enumerate((0.0, 2.0 ** -10, 0.5)):
        beta_t = torch.tensor(beta, dtype=torch.float32, device=dev)
        total, gscale = 2 * S, 0.5
        counter = torch.zeros(1, dtype=torch.int32, device=dev)
        res, out, sums, sc, ticket = run_final(dev, form, S, B, N, K, mode, tg, ticketed, counter=counter, seed=S,
                                               loss=dict(beta=beta_t, total_samples=total, grad_scale=gscale))
        out4, g_a, g_b, g_kl3, g_lg = (np64(t_) for t_ in out["loss"])
        lg = res["y"].cpu().numpy()
        nll_got = np64(out["nll"])
        what = f"{form} S={S} ticket={ticketed} beta={beta}"
        check_nll(out["nll"], lg, tg, mode, what + " nll")
        a = np64(out["kl"] if lr else out["log_prior"])
        b = None if lr else np64(out["log_q"])
        want = R.loss_assembly(a, b, nll_got, beta, total, gscale, lr)
        tol = R.loss_assembly_tol(a, b, nll_got, beta, total, gscale, lr)
        for name, g_, w_, t_ in zip(("out4", "g_a", "g_b", "g_kl3"), (out4, g_a, g_b, g_kl3), want, tol):
            R.assert_close(g_, w_, t_, f"{what} {name}")
        gs = gscale / total
        R.assert_close(g_lg, R.nll_grad(lg, tg, mode, SIGMA, gs), R.nll_grad_tol(lg, tg, mode, SIGMA, gs), what + " g_logits")
        assert int(counter.item()) == S, what + " counter"
        assert ticket is None or int(ticket.item()) == 0
        check_form(form, sc, S, B, N, ticketed, True)


# ------------------------------------------------------------------------------------------------------ 6. gradient kernels
@pytest.mark.parametrize("mode,C,B,S,ticketed,offset", [c for c in K4_CASES if not c[5] and c[2] * c[3] * c[1] <= 600000],
                         ids=[f"{c[0][:3]}-C{c[1]}-B{c[2]}-S{c[3]}" for c in K4_CASES if not c[5] and c[2] * c[3] * c[1] <= 600000])
def test_nll_backward_kernels_against_fp64(dev, mode, C, B, S, ticketed, offset):
    lg, tg = inputs(mode, S, B, C, 600 + C)
    lg_t, tgt = torch.from_numpy(lg).to(dev), dev_target(tg, dev)
    rs = np.random.RandomState(C)
    g = rs.uniform(0.2, 1.0, S).astype(np.float32)
    got = ops.nll_bwd(lg_t, tgt, torch.from_numpy(g).to(dev), mode, SIGMA)
    R.assert_close(np64(got), R.nll_grad(lg, tg, mode, SIGMA, g), R.nll_grad_tol(lg, tg, mode, SIGMA, g), "nll_bwd")
    a, b, n = (torch.from_numpy(rs.standard_normal(S).astype(np.float32) * 100).to(dev) for _ in range(3))
    beta = torch.tensor(0.37, device=dev)
    o4, ga, gb, gk, gl = ops.elbo_loss_nll_bwd(a, b, n, beta, 2 * S, False, lg_t, tgt, mode, SIGMA, grad_scale=0.5)
    gs = 0.5 / (2 * S)
    R.assert_close(np64(gl), R.nll_grad(lg, tg, mode, SIGMA, gs), R.nll_grad_tol(lg, tg, mode, SIGMA, gs), "elbo_loss_nll_bwd")
    args = (np64(a), np64(b), np64(n), 0.37, 2 * S, 0.5, False)
    for name, g_, w_, t_ in zip(("out4", "g_a", "g_b", "g_kl3"), (o4, ga, gb, gk), R.loss_assembly(*args), R.loss_assembly_tol(*args)):
        R.assert_close(np64(g_), w_, t_, name)


# ------------------------------------------------------------------------------------------------------ 7. bad labels
@pytest.mark.parametrize("C,B,S,ticketed,scratch", [(1, 17, 1, False, False), (10, 17, 4, True, False), (16, 9, 65, False, False),
                                                    (17, 128, 2, False, False), (100, 37, 17, True, False),
                                                    (1000, 33, 2, False, True)])
def test_bad_labels_poison_only_their_rows_k4(dev, C, B, S, ticketed, scratch):
    """K4 (every fin_nll branch, nll_rows_kernel) and both gradient kernels: labels -1 and C poison their rows only.
    One shared target: every sample's NLL is NaN.  Per-group targets: only the bad group's samples are."""
    mode = "classification"
    for per_group in (False, True):
        G = 1 if not per_group else (S if S > 1 else 1)
        lg, tg = inputs(mode, S, B, C, 700 + C, groups=G)
        tg[-1, 1 % B] = -1
        tg[-1, (B - 2) % B] = C
        lg_t, tgt = torch.from_numpy(lg).to(dev), dev_target(tg, dev)
        sc = sentinel_scratch(S, dev) if scratch else None
        ticket = torch.zeros(1, dtype=torch.int32, device=dev) if ticketed else None
        out = k4_call(dev, lg_t, tgt, mode, S, group_samples=(1 if per_group and G > 1 else 0), ticket=ticket, scratch=sc)
        check_nll(out["nll"], lg, tg, mode, f"per_group={per_group}")  # NaN exactly for the samples that read the bad block
        if not per_group:
            g = ops.nll_bwd(lg_t, tgt, torch.ones(S, device=dev), mode)
            R.assert_close(np64(g), R.nll_grad(lg, tg, mode), R.nll_grad_tol(lg, tg, mode), "nll_bwd")
            z = torch.zeros(S, device=dev)
            gl = ops.elbo_loss_nll_bwd(z, z, z, torch.tensor(0.5, device=dev), S, False, lg_t, tgt, mode)[4]
            R.assert_close(np64(gl), R.nll_grad(lg, tg, mode, gs=1.0 / S), R.nll_grad_tol(lg, tg, mode, gs=1.0 / S), "fused bwd")


@pytest.mark.parametrize("form,S", [("k1c", 4), ("k1c", 17), ("k1r", 3), ("k1r", 65), ("k3r", 2), ("k3r_prep", 65)])
def test_bad_labels_poison_only_their_rows_fused(dev, form, S):
    """The inline NLL of K1c / K1r / K3r and fin_loss_row_grad: the bad rows' gradient is NaN, every other gradient row,
    the complexity scalars and the seeds stay finite and correct; the NLL, and with it out4[0] / out4[3], is NaN."""
    B, N, mode = 17, 10, "classification"
    tg = R.make_labels(B, N, 800)
    tg[0, 3], tg[0, 11] = -1, N
    lr = form.startswith("k3r")
    res, out, sums, sc, ticket = run_final(dev, form, S, B, N, 512 if form == "k1c" else 96, mode, tg, True, seed=S,
                                           loss=dict(beta=torch.tensor(0.5, device=dev), total_samples=S, grad_scale=1.0))
    lg = res["y"].cpu().numpy()
    check_nll(out["nll"], lg, tg, mode, form)
    assert np.isnan(np64(out["nll"])).all()
    g_lg = np64(out["loss"][4])
    R.assert_close(g_lg, R.nll_grad(lg, tg, mode, gs=1.0 / S), R.nll_grad_tol(lg, tg, mode, gs=1.0 / S), form + " g_logits")
    a = np64(out["kl"] if lr else out["log_prior"])
    assert np.isfinite(a).all() and np.isfinite(np64(out["loss"][1])).all() and np.isfinite(np64(out["loss"][2])).all()
    o4 = np64(out["loss"][0])
    assert np.isnan(o4[[0, 3]]).all() and np.isfinite(o4[1:3]).all()
    assert tickets_zero(sc, S) and int(ticket.item()) == 0


# ------------------------------------------------------------------------------------------------------ 8. end to end
def build(dev, variant, classes, dims_in=48, hidden=40, B=37):
    import networks
    lr, mix = variant == "lr", variant == "mix"
    prior_init = [0.5, -1.0, -6.0] if mix else [1.0]
    mp = dict(input_shape=dims_in, classes=classes, batch_size=B, hidden_units=hidden, mode="classification",
              mu_init=[-0.2, 0.2], rho_init=[-5, -4], prior_init=prior_init, mixture_prior=mix, local_reparam=lr)
    net = networks.BayesianNetwork(mp)
    sd = synth.synth_state_dict(dims_in, hidden, classes, lr)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    p = O.NetParams.from_state_dict(sd, "classification", dims_in, lr, O.Prior.from_init(prior_init, mix))
    return net.to(dev).train(), p, sd


@pytest.mark.parametrize("classes", [2, 17, 33, 100])
@pytest.mark.parametrize("variant", ["bbb", "mix", "lr"])
def test_drop_in_network_at_other_class_counts(dev, variant, classes):
    """networks.BayesianNetwork with 2 / 17 / 33 / 100 classes, f32 math, on-chip Philox: sample_elbo(_lr) against the
    oracle on the same epsilon (oracle.philox_eps_for_network) at the fp32 timed-path tolerances (statistics 1e-5, NLL
    2e-5, ELBO 1e-4); for 17 and 100 classes also the parameter gradients of one step against float64 autograd."""
    lr = variant == "lr"
    S, B, seed, first, beta = 3, 37, 9090 + classes, 500, 0.25
    net, p, sd = build(dev, variant, classes, B=B)
    x, y = synth.synth_batch("classification", B, 48, classes, seed=classes)
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    bnn_hip.manual_seed(seed, counter=first)
    net.zero_grad()
    got = (net.sample_elbo_lr if lr else net.sample_elbo)(xd, yd, beta, S)
    eps = [O.philox_eps_for_network(p, B, seed, first + j) for j in range(S)]
    ref = (O.sample_elbo_lr if lr else O.sample_elbo)(p, torch.from_numpy(x), torch.from_numpy(y), beta, S, eps=eps)
    g = [float(v.detach().double().cpu().reshape(-1)[0]) for v in got]
    r = [float(v.double().reshape(-1)[0]) for v in ref]
    for i, (u, w) in enumerate(zip(g, r)):
        rtol = 1e-4 if i == 0 else (2e-5 if i == len(g) - 1 else 1e-5)
        assert abs(u - w) <= rtol * abs(w), (i, u, w)
    if classes not in (17, 100):
        return
    got[0].backward()
    # float64 autograd through the oracle on the same epsilon
    layers = [tuple(t.detach().double().requires_grad_(True) for t in l) for l in p.layers]
    p64 = O.NetParams(layers, p.mode, p.input_shape, p.local_reparam, p.prior)
    x64 = torch.from_numpy(x).double()
    a_s, b_s, n_s = 0, 0, 0
    for j in range(S):
        out, a_, b_ = O.network_forward(p64, x64, [e.double() for e in eps[j]])
        a_s, b_s = a_s + a_, b_s + (b_ if b_ is not None else 0)
        n_s = n_s + O.nll(out, torch.from_numpy(y), "classification")
    b32 = float(np.float32(beta))
    loss = (b32 * a_s / S + n_s / S) if lr else (b32 * b_s / S - b32 * a_s / S + n_s / S)
    loss.backward()
    mods = (net.l1, net.l2, net.l3)
    for li, m in enumerate(mods):
        for k, name in enumerate(("weight_mu", "weight_rho", "bias_mu", "bias_rho")):
            gg = getattr(m, name).grad.detach().double().cpu().numpy()
            ww = layers[li][k].grad.numpy()
            scale = np.abs(ww).max() + 1e-30
            assert np.abs(gg - ww).max() <= 1e-4 * scale, (li, name, np.abs(gg - ww).max(), scale)
