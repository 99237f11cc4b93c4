"""Piece-order operands of the pair block GEMM (K1b2; include/bnn_hip.h, bnn_layout and bnn_bbb_fwd_args.w_pieces): every
comparison is BIT equality between the piece-order path and the same library's row-major path.  The index maps of the layouts
are restated here from their definitions and not taken from the package: activations [row][batch block of 128][k-step t]
[batch tile m][lane][8 bf16], lane (r = lane & 15, q = lane >> 4) of piece (t, m) holding x[128 block + 16 m + r][32 t + 8 q .. + 7];
parameters [feature tile T][k-step t][mu lo | mu hi | sigma lo | sigma hi][lane][4 fp32], lane (r, q) holding
mu | sigma [16 T + r][32 t + 8 q + 0..3] (lo) and + 4..7 (hi); both zero-padded."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bnn_hip
from bnn_hip import _lib as L
from bnn_hip import engine, ops, synth

ERR_ENUM = -3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _bf16_math():
    bnn_hip.set_math("bf16")
    yield
    bnn_hip.set_math("bf16")


def piece_index(shape):
    """int64 [rows, B, K]: the position (in bf16 elements) of every logical element in the piece-order buffer, and the
    buffer's length."""
    rows, B, K = shape if len(shape) == 3 else (1,) + tuple(shape)
    mbs, ks = (B + 127) // 128, (K + 31) // 32
    row = np.arange(rows, dtype=np.int64)[:, None, None]
    b = np.arange(B, dtype=np.int64)[None, :, None]
    k = np.arange(K, dtype=np.int64)[None, None, :]
    blk, m, r = b // 128, (b % 128) // 16, b % 16
    t, q, e = k // 32, (k % 32) // 8, k % 8
    lane = q * 16 + r
    return ((((row * mbs + blk) * ks + t) * 8 + m) * 64 + lane) * 8 + e, rows * mbs * ks * 8 * 64 * 8


def to_pieces(x):
    """Host re-ordering of a row-major bf16 tensor: the raw bits (int16) of the piece-order buffer, pads zero."""
    idx, n = piece_index(tuple(x.shape))
    buf = np.zeros(n, dtype=np.int16)
    buf[idx.reshape(-1)] = x.detach().cpu().contiguous().view(torch.int16).numpy().reshape(-1)
    return torch.from_numpy(buf)


def params_to_pieces(mu, sigma):
    """Host re-ordering of the row-major fp32 [N, K] (mu, sigma): the raw bits (int32) of the parameter pieces, pads zero."""
    N, K = mu.shape
    T, ks = (N + 15) // 16, (K + 31) // 32
    n = np.arange(N, dtype=np.int64)[:, None]
    k = np.arange(K, dtype=np.int64)[None, :]
    tile, r, t, q, h, e = n // 16, n % 16, k // 32, (k % 32) // 8, (k % 8) // 4, k % 4
    buf = np.zeros(T * ks * 4 * 64 * 4, dtype=np.int32)
    for first, src in ((0, mu), (2, sigma)):
        idx = ((((tile * ks + t) * 4 + first + h) * 64 + q * 16 + r) * 4 + e).reshape(-1)
        buf[idx] = src.detach().cpu().contiguous().view(torch.int32).numpy().reshape(-1)
    return torch.from_numpy(buf)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).reshape(-1)


def pieces_of(x, dev):
    """A piece-order device buffer holding the row-major bf16 tensor x."""
    buf = ops.pieces_activation(tuple(x.shape), dev)
    buf.view(torch.int16).view(-1).copy_(to_pieces(x).to(dev))
    return buf


def layer(K, N, seed, dev):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    wm = ((torch.rand((N, K), generator=gen) - 0.5) * 0.4).to(dev)
    wr = (torch.rand((N, K), generator=gen) - 5.0).to(dev)
    bm = ((torch.rand(N, generator=gen) - 0.5) * 0.4).to(dev)
    br = (torch.rand(N, generator=gen) - 5.0).to(dev)
    return wm, wr, bm, br


SHAPES = [(4, 128, 64, 64),      # all full
          (5, 100, 40, 72),      # odd pair count (a last block with one active pair), short batch rows, an 8-k tail step, a partial
                                 # feature tile, phantom waves
          (4, 128, 784, 80)]     # the first layer's tail of 16 k


@pytest.fixture(scope="module")
def row_major(dev):
    """Per shape: the inputs and the row-major launch's results (computed once, never modified)."""
    res = {}
    for S, B, K, N in SHAPES:
        gen = torch.Generator(device="cpu").manual_seed(S * 1000 + K + N)
        x16 = (torch.rand(S, B, K, generator=gen) - 0.3).to(torch.bfloat16).to(dev)
        w = layer(K, N, K * 7 + N, dev)
        kw = dict(n_samples=S, prior=ops.PriorSpec(False, 0.9), math_mode=L.MATH_BF16, relu=True, y_dtype=torch.bfloat16,
                  eps_mode=L.EPS_PHILOX, seed=41, layer_id=1, sample_offset=3, want_stats=True, want_scalars=True, dump_eps=True,
                  form=L.FORM_GEMM, w_sigma=ops.softplus(w[1]))
        plan = ops.bbb_plan(x16, *w, **kw)
        assert plan["form"] == L.FORM_GEMM and plan["waves"] == 8          # the pair block GEMM
        res[(S, B, K, N)] = (x16, w, kw, plan, ops.bbb_linear_fwd(x16, *w, **kw))
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("x_pieces,y_pieces,w_pieces", [(True, False, False), (False, True, False), (True, True, False),
                                                        (False, False, True), (True, True, True)])
def test_one_launch_equals_the_row_major_launch(dev, row_major, shape, x_pieces, y_pieces, w_pieces):
    """K1b2 with x and / or y and / or its parameters in piece order: y (un-tiled here), the per-sample scalars and the epsilon it
    drew equal the row-major launch's bit for bit, the plan is the same, and the pad positions of a piece-order y are still zero."""
    S, B, K, N = shape
    x16, w, kw, plan, ref = row_major[shape]
    xin = pieces_of(x16, dev) if x_pieces else x16
    out = ops.pieces_activation((S, B, N), dev) if y_pieces else None
    wp = None
    if w_pieces:
        wp = ops.param_pieces(N, K, dev)
        wp.view(torch.int32).view(-1).copy_(params_to_pieces(w[0], kw["w_sigma"]).to(dev))
    assert ops.bbb_plan(xin, *w, out=out, w_pieces=wp, **kw) == plan
    got = ops.bbb_linear_fwd(xin, *w, out=out, w_pieces=wp, **kw)
    if y_pieces:
        assert got["y"] is out
        # the whole buffer against the host re-ordering of the row-major y: the values AND the zero pads
        assert torch.equal(bits(out), to_pieces(ref["y"]))
        assert torch.equal(bits(ops.unpiece(out)), bits(ref["y"]))
    else:
        assert torch.equal(bits(got["y"]), bits(ref["y"]))
    for k in ("log_prior", "log_q", "eps_w", "eps_b"):
        assert torch.equal(bits(got[k]), bits(ref[k])), k


@pytest.mark.parametrize("shape", [(2, 100, 40), (3, 128, 784), (130, 72)])
def test_prepare_casts_into_piece_order(dev, shape):
    """eval_prepare's bf16 cast written in piece order = the host re-ordering of its row-major output (same rounding), pads zero;
    the hoisted sigma beside it is untouched by the option."""
    gen = torch.Generator(device="cpu").manual_seed(sum(shape))
    x = ((torch.rand(*shape, generator=gen) - 0.5) * 3.0).to(dev)
    rho = (torch.rand((72, shape[-1]), generator=gen) - 5.0).to(dev)
    sig_r, c_r, _ = ops.eval_prepare([rho], cast=x)
    buf = ops.pieces_activation(shape, dev)
    sig_p, c_p, _ = ops.eval_prepare([rho], cast=x, cast_out=buf)
    assert c_p is buf
    assert torch.equal(bits(buf), to_pieces(c_r))
    assert torch.equal(bits(sig_p[0]), bits(sig_r[0]))
    # the (mu, sigma) of a 72 x K layer in piece order, beside the row-major sigma and the cast
    mu = ((torch.rand(rho.shape, generator=gen) - 0.5) * 0.4).to(dev)
    wp, buf2 = ops.param_pieces(72, shape[-1], dev), ops.pieces_activation(shape, dev)
    sig_q, _, _ = ops.eval_prepare([rho], cast=x, cast_out=buf2, mus=[mu], pieces=[wp])
    assert torch.equal(bits(wp), params_to_pieces(mu, sig_r[0]))
    assert torch.equal(bits(sig_q[0]), bits(sig_r[0])) and torch.equal(bits(buf2), bits(buf))


def test_chain_of_two_layers_equals_the_row_major_chain(dev):
    """Layer 1 writing piece order into layer 2 reading it = the row-major chain, at widths 40-72-72 (tail steps on both sides)."""
    S, B = 5, 100
    gen = torch.Generator(device="cpu").manual_seed(9)
    x16 = (torch.rand(S, B, 40, generator=gen) - 0.3).to(torch.bfloat16).to(dev)
    w1, w2 = layer(40, 72, 1, dev), layer(72, 72, 2, dev)

    def kw(w, lid):
        return dict(n_samples=S, prior=ops.PriorSpec(False, 1.0), math_mode=L.MATH_BF16, relu=True, y_dtype=torch.bfloat16,
                    eps_mode=L.EPS_PHILOX, seed=5, layer_id=lid, sample_offset=0, want_stats=True, want_scalars=True,
                    form=L.FORM_GEMM, w_sigma=ops.softplus(w[1]))
    h_r = ops.bbb_linear_fwd(x16, *w1, **kw(w1, 0))
    y_r = ops.bbb_linear_fwd(h_r["y"], *w2, **kw(w2, 1))
    h_p = ops.bbb_linear_fwd(pieces_of(x16, dev), *w1, out=ops.pieces_activation((S, B, 72), dev), **kw(w1, 0))
    assert ops.bbb_plan(h_p["y"], *w2, **kw(w2, 1))["waves"] == 8
    y_p = ops.bbb_linear_fwd(h_p["y"], *w2, **kw(w2, 1))
    assert torch.equal(bits(y_p["y"]), bits(y_r["y"]))
    for k in ("log_prior", "log_q"):
        assert torch.equal(bits(h_p[k]), bits(h_r[k])) and torch.equal(bits(y_p[k]), bits(y_r[k]))


def test_stacked_evaluator_equals_itself_without_piece_order(dev, monkeypatch):
    """A stacked GraphedElbo whose hidden layers launch K1b2 (asserted from the plan): sums, logits and the per-pair scalars equal
    the same evaluator with the piece-order layouts switched off, replay after replay, and consecutive replays draw fresh epsilon."""
    import networks
    dims, G, B = (40, 72, 10), 6, 100
    monkeypatch.setattr(bnn_hip.runtime.state, "form", L.FORM_GEMM)
    monkeypatch.setattr(engine, "SPLIT_MIN_WEIGHTS", 0)            # hoist sigma on this small network too: K1b2 needs it
    mp = dict(input_shape=dims[0], classes=dims[2], batch_size=B, hidden_units=dims[1], mode="classification",
              mu_init=[-0.2, 0.2], rho_init=[-5, -4], prior_init=[1.0], mixture_prior=False, local_reparam=False)
    net = networks.BayesianNetwork(mp)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(*dims, False).items()})
    net.to(dev).train()
    xs, ys = zip(*(synth.synth_batch("classification", B, dims[0], dims[2], seed=g) for g in range(G)))
    x = torch.from_numpy(np.stack(xs)).to(dev)
    y = torch.from_numpy(np.stack(ys)).to(dev)
    runs = {}
    for pieces in (True, False):
        monkeypatch.setattr(bnn_hip.runtime.state, "pieces", pieces)
        monkeypatch.setattr(bnn_hip.runtime.state, "param_pieces", pieces)
        bnn_hip.manual_seed(321, counter=50)
        ev = engine.GraphedElbo(net, x, y, 1, stacked=True)
        assert ev.k1b2 == ([True, True, False] if pieces else [False] * 3)
        assert (ops.pieces_shape(ev.x16) is not None) == pieces and (ops.pieces_shape(ev.bufs[0]) is not None) == pieces
        assert ops.pieces_shape(ev.bufs[1]) is None                 # the output layer reads row-major activations
        assert [w is not None for w in ev.wpieces] == ev.k1b2
        p2 = tuple(t.detach() for t in (net.l2.weight_mu, net.l2.weight_rho, net.l2.bias_mu, net.l2.bias_rho))
        plan = ops.bbb_plan(ev.bufs[0], *p2, **ev._bbb_kw(1, ev.bufs[0], None, ev._common_kw(1)))
        assert plan["form"] == L.FORM_GEMM and plan["waves"] == 8
        reps = []
        for _ in range(2):
            ev.replay()
            torch.cuda.synchronize()
            reps.append({"sums": ev.sums.clone(), "logits": ev.logits.clone(), **{k: v.clone() for k, v in ev.out.items()}})
        runs[pieces] = reps
    for a, b in zip(runs[True], runs[False]):
        for k in a:
            assert torch.equal(bits(a[k]), bits(b[k])), k
    assert not torch.equal(runs[True][0]["logits"], runs[True][1]["logits"])


def test_other_plans_refuse_piece_order_operands(dev, row_major):
    """A piece-order operand handed to a launch whose plan is not K1b2 in bf16 math returns BNN_ERR_ENUM and launches nothing;
    the plan itself does not depend on the layout flags (headline shape: 19 x 128 blocks of 8 waves, 66 048 B of LDS)."""
    S, B, K, N = SHAPES[0]
    x16, w, kw, plan, ref = row_major[SHAPES[0]]
    xin, out = pieces_of(x16, dev), ops.pieces_activation((S, B, N), dev)

    def refused(x, o, **over):
        with pytest.raises(ops.BnnHipError, match=f"status {ERR_ENUM} "):
            ops.bbb_linear_fwd(x, *w, out=o, **{**kw, **over})
    wp = ops.param_pieces(N, K, dev)
    for x, o, pc in ((xin, None, None), (x16, out, None), (x16, None, wp)):
        refused(x, o, form=L.FORM_TILE, w_pieces=pc)                      # K1a
        if pc is None:
            refused(x, o, w_sigma=None)                                   # K1b (no hoisted sigma: parameters in registers)
        refused(x, o, math_mode=L.MATH_F32, form=L.FORM_AUTO, w_pieces=pc)    # fp32 math
        refused(x, o, form=L.FORM_GEMM_KSLICE, split_scratch=ops.split_scratch(S, B, N, dev), w_pieces=pc)     # K-sliced
    # split-bf16 math: the form's operands are plane pairs -- refused as well
    lo = torch.zeros_like(xin)
    lo.bnn_pieces = xin.bnn_pieces
    with pytest.raises(ops.BnnHipError, match=f"status {ERR_ENUM} "):
        ops.bbb_linear_fwd(xin, *w, **{**kw, "math_mode": L.MATH_BF16X3, "x_lo": lo})
    # the matmul-only form over pre-sampled weights, and the local-reparameterisation layer's binding
    ws = torch.zeros((S, N, K), dtype=torch.bfloat16, device=dev)
    with pytest.raises(ops.BnnHipError, match=f"status {ERR_ENUM} "):
        ops.bbb_sampled_matmul(xin, ws, torch.zeros((S, N), device=dev), n_samples=S, relu=True, y_dtype=torch.bfloat16)
    with pytest.raises(ops.BnnHipError, match="piece-order"):
        ops.lr_linear_fwd(xin, *w, n_samples=S, sigma_p=1.0, math_mode=L.MATH_BF16, relu=True, y_dtype=torch.bfloat16,
                          eps_mode=L.EPS_PHILOX)
    torch.cuda.synchronize()
    assert not bool(out.view(torch.int16).any())                          # nothing was written

    lib = L.load()
    P = 0x10000                                                           # plans never dereference

    def headline(xl, yl, wpc=None):
        a = L.BbbFwdArgs()
        a.struct_bytes = C.sizeof(L.BbbFwdArgs)
        a.n_samples, a.batch, a.in_features, a.out_features = 256, 128, 1200, 1200
        a.x = a.w_mu = a.w_rho = a.b_mu = a.b_rho = a.y = a.w_sigma = P
        a.x_dtype, a.y_dtype, a.math, a.x_per_sample = L.BF16, L.BF16, L.MATH_BF16, 1
        a.prior.sigma_p = 1.0
        a.x_layout, a.y_layout, a.w_pieces = xl, yl, wpc
        pl = L.Plan()
        assert lib.bnn_bbb_plan(C.byref(a), C.byref(pl)) == 0
        return (pl.form, pl.waves, pl.blocks, pl.lds_bytes)
    assert headline(0, 0) == (L.FORM_GEMM, 8, 19 * 128, 66048)
    for xl, yl, wpc in ((1, 0, None), (0, 1, None), (1, 1, None), (0, 0, P), (1, 1, P)):
        assert headline(xl, yl, wpc) == headline(0, 0)
