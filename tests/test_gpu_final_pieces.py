"""The one-launch output layer (K1c: bnn_bbb_final_fwd's fused form) reading its x in PIECE ORDER (include/bnn_hip.h, bnn_layout),
alone, behind a K1b2 launch that writes the layout, and inside a stacked GraphedElbo: every comparison is BIT equality with the same
library's row-major path.  The piece-order buffers are filled with the host re-ordering of test_gpu_tiled_operands (restated there
from the layout's definition, not taken from the package).  A piece-order x handed to any other output-layer form is refused with
BNN_ERR_ENUM -- so a call over such an x that succeeds has run K1c."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bnn_hip
from bnn_hip import _lib as L
from bnn_hip import engine, ops, synth
from test_gpu_tiled_operands import bits, layer, pieces_of, to_pieces

ERR_ENUM = -3
PRIOR = ops.PriorSpec(False, 0.9)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _bf16_math():
    bnn_hip.set_math("bf16")
    yield
    bnn_hip.set_math("bf16")


def final(x, w, S, B, K, N, dev, mode="classification", below=None, **over):
    """One bnn_bbb_final_fwd call over x ([S, B, K] row-major or its piece-order buffer), every buffer it writes allocated ZEROED
    here.  18 pairs and more run as the headline group does (one minibatch per pair: [S, 4] sums behind the sums launch), fewer
    as the MC samples of one minibatch (the ticket path).  `below` = (workspace, K, N) of a hidden layer under it.
    Returns every result as a dict of tensors."""
    groups = S > 16
    gen = torch.Generator(device="cpu").manual_seed(S * 31 + B)
    lead = (S, B) if groups else (B,)
    if mode == "classification":
        target = torch.randint(0, N, lead, generator=gen).to(dev)
    else:
        target = torch.rand(lead + (N,), generator=gen).to(dev)
    counter = torch.tensor([7], dtype=torch.int32, device=dev)
    sums = torch.zeros((S if groups else 1, 4), dtype=torch.float32, device=dev)
    ws = torch.zeros_like(ops.bbb_workspace(S, N, dev))
    grp = dict(sample_group=1, sample_group_stride=1) if groups else {}
    layer_kw = dict(n_samples=S, prior=PRIOR, math_mode=L.MATH_BF16, relu=False, y_dtype=torch.float32, eps_mode=L.EPS_PHILOX, seed=41,
                    layer_id=2, sample_offset=3, want_stats=True, sample_counter=counter, workspace=ws,
                    out=torch.zeros((S, B, N), dtype=torch.float32, device=dev), **grp)
    layer_kw.update(over)
    lows = [below] if below is not None else []
    fin_kw = dict(workspaces=[b[0] for b in lows], layer_in=[b[1] for b in lows] + [K], layer_out=[b[2] for b in lows] + [N],
                  local_reparam=False, prior=PRIOR, n_samples=S, target=target, mode=mode, nll_sigma=0.7, sample_counter=counter,
                  sample_counter_inc=S, sums=sums, ticket=torch.zeros(1, dtype=torch.int32, device=dev),
                  scratch=ops.final_scratch(S, dev), group_samples=1 if groups else 0,
                  out={k: torch.zeros(S, dtype=torch.float32, device=dev) for k in ("log_prior", "log_q", "nll")})
    res, out = ops.bbb_final_fwd((x,) + tuple(w), layer_kw, fin_kw)
    torch.cuda.synchronize()
    return dict(logits=res["y"], workspace=ws, sums=sums, counter=counter, log_prior=out["log_prior"], log_q=out["log_q"], nll=out["nll"])


def assert_same_bits(got, ref):
    for k in ref:
        assert torch.equal(bits(got[k]), bits(ref[k])), k


def x_of(S, B, K, dev, seed):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(S, B, K, generator=gen) - 0.3).to(torch.bfloat16).to(dev)


# (K, N, B, S, mode): one k-step pair; a k tail inside a step (40 = 32 + 8: the lanes q >= 1 of step 1 read zero pads); the headline
# output layer, 38 k-steps in 5 K-range slices per pair (18 x 5 <= 128 blocks: the sliced form); ragged rows on a regression head
# (rows 100 .. 127 of the piece-order buffer are zeros, where the row-major path clamps the row)
K1C_SHAPES = [(64, 10, 128, 1, "classification"), (40, 10, 128, 3, "classification"), (1200, 10, 128, 18, "classification"),
              (72, 1, 100, 2, "regression")]


@pytest.mark.parametrize("K,N,B,S,mode", K1C_SHAPES)
def test_k1c_over_a_piece_order_x_equals_the_row_major_launch(dev, K, N, B, S, mode):
    """K1c alone: logits, per-sample log p / log q / NLL, the sums, the statistics workspace and the advanced sample counter."""
    x16 = x_of(S, B, K, dev, K + N + S)
    w = layer(K, N, K * 3 + N, dev)
    ref = final(x16, w, S, B, K, N, dev, mode)
    got = final(pieces_of(x16, dev), w, S, B, K, N, dev, mode)
    assert int(ref["counter"].item()) == 7 + S and bool(ref["logits"].abs().sum() > 0) and bool(ref["nll"].abs().sum() > 0)
    assert_same_bits(got, ref)


@pytest.mark.parametrize("N1", [80, 64])
@pytest.mark.parametrize("B", [128, 100])
def test_k1b2_writing_piece_order_into_k1c(dev, N1, B):
    """A forced block-GEMM hidden layer (K1b2, asserted from the plan) writing y in piece order, K1c reading it: equal to the
    row-major pair of launches, and the hidden buffer is the host re-ordering of the row-major y -- values and zero pads.  80
    features: a phantom wave and a masked feature tile on the writing side, a 16-k tail step on the reading side."""
    S, K = 5, 64
    x16 = x_of(S, B, K, dev, N1 + B)
    w1, w2 = layer(K, N1, 11, dev), layer(N1, 10, 12, dev)
    kw = dict(n_samples=S, prior=PRIOR, math_mode=L.MATH_BF16, relu=True, y_dtype=torch.bfloat16, eps_mode=L.EPS_PHILOX, seed=41,
              layer_id=1, sample_offset=3, want_stats=True, form=L.FORM_GEMM, w_sigma=ops.softplus(w1[1]))
    plan = ops.bbb_plan(x16, *w1, **kw)
    assert plan["form"] == L.FORM_GEMM and plan["waves"] == 8
    ws_r, ws_p = (torch.zeros_like(ops.bbb_workspace(S, N1, dev)) for _ in range(2))
    h_r = ops.bbb_linear_fwd(x16, *w1, workspace=ws_r, **kw)
    ref = final(h_r["y"], w2, S, B, N1, 10, dev, below=(ws_r, K, N1))
    buf = ops.pieces_activation((S, B, N1), dev)
    h_p = ops.bbb_linear_fwd(x16, *w1, workspace=ws_p, out=buf, **kw)
    assert h_p["y"] is buf
    got = final(buf, w2, S, B, N1, 10, dev, below=(ws_p, K, N1))
    assert_same_bits(got, ref)
    assert torch.equal(bits(ws_p), bits(ws_r))
    assert torch.equal(bits(buf), to_pieces(h_r["y"]))          # after both launches: the pads are still zero


class _HiddenBlockGemm(engine.GraphedElbo):
    """GraphedElbo with the block-GEMM preference on the HIDDEN layers only: a small network then launches K1b2 there, and its
    output layer keeps the library's own choice (the one-launch form is taken without a preference only)."""

    def _common_kw(self, i):
        kw = super()._common_kw(i)
        if i < len(self.specs) - 1:
            kw["form"] = L.FORM_GEMM
        return kw


def _small_net(dev, dims, B, G):
    import networks
    mp = dict(input_shape=dims[0], classes=dims[2], batch_size=B, hidden_units=dims[1], mode="classification",
              mu_init=[-0.2, 0.2], rho_init=[-5, -4], prior_init=[1.0], mixture_prior=False, local_reparam=False)
    net = networks.BayesianNetwork(mp)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(*dims, False).items()})
    net.to(dev).train()
    xs, ys = zip(*(synth.synth_batch("classification", B, dims[0], dims[2], seed=g) for g in range(G)))
    return net, torch.from_numpy(np.stack(xs)).to(dev), torch.from_numpy(np.stack(ys)).to(dev)


def test_stacked_evaluator_hands_piece_order_to_k1c(dev, monkeypatch):
    """A stacked GraphedElbo of 18 minibatches on a 40-80-80-10 network, hidden layers K1b2 and output layer K1c (both asserted):
    sums, logits and the per-pair scalars of two replays equal those of the same evaluator with only the new hand-over switched
    off, and with every piece-order layout switched off."""
    dims, G, B = (40, 80, 10), 18, 128
    monkeypatch.setattr(engine, "SPLIT_MIN_WEIGHTS", 0)            # hoist sigma on this small network too: K1b2 needs it
    net, x, y = _small_net(dev, dims, B, G)
    runs = {}
    for pieces, final_pieces in ((True, True), (True, False), (False, False)):
        monkeypatch.setattr(bnn_hip.runtime.state, "pieces", pieces)
        monkeypatch.setattr(bnn_hip.runtime.state, "param_pieces", pieces)
        monkeypatch.setattr(bnn_hip.runtime.state, "final_pieces", final_pieces)
        bnn_hip.manual_seed(321, counter=50)
        ev = _HiddenBlockGemm(net, x, y, 1, stacked=True)
        assert ev.k1b2 == ([True, True, False] if pieces else [False] * 3)
        assert ev.k1c and not ev.rows                                # more pairs than the row-split form takes, one tile, <= 128 rows
        assert [ops.pieces_shape(t) is not None for t in (ev.x16, ev.bufs[0], ev.bufs[1])] == [pieces, pieces, final_pieces]
        assert ops.pieces_shape(ev.bufs[2]) is None
        p2 = tuple(t.detach() for t in (net.l2.weight_mu, net.l2.weight_rho, net.l2.bias_mu, net.l2.bias_rho))
        plan = ops.bbb_plan(ev.bufs[0], *p2, **ev._bbb_kw(1, ev.bufs[0], None, ev._common_kw(1)))
        assert plan["form"] == L.FORM_GEMM and plan["waves"] == 8   # (K1c: a piece-order x is refused by every other output-layer form)
        reps = []
        for _ in range(2):
            ev.replay()
            torch.cuda.synchronize()
            reps.append({"sums": ev.sums.clone(), "logits": ev.logits.clone(), **{k: v.clone() for k, v in ev.out.items()}})
        runs[(pieces, final_pieces)] = reps
    for other in ((True, False), (False, False)):
        for a, b in zip(runs[(True, True)], runs[other]):
            for k in a:
                assert torch.equal(bits(a[k]), bits(b[k])), (other, k)
    assert not torch.equal(runs[(True, True)][0]["logits"], runs[(True, True)][1]["logits"])


def test_row_split_output_layer_keeps_a_row_major_buffer(dev, monkeypatch):
    """8 minibatches: the output layer takes the row-split form over pre-sampled weights (K1r) -- its input stays row-major."""
    monkeypatch.setattr(engine, "SPLIT_MIN_WEIGHTS", 0)
    net, x, y = _small_net(dev, (40, 80, 10), 128, 8)
    bnn_hip.manual_seed(321, counter=50)
    ev = _HiddenBlockGemm(net, x, y, 1, stacked=True)
    assert ev.rows and not ev.k1c and ev.k1b2[0]
    assert ops.pieces_shape(ev.bufs[0]) is None and ops.pieces_shape(ev.bufs[1]) is None      # (layer 2 carries the sampling rider: not K1b2)
    ev.replay()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ev.sums).all())


def test_other_output_layer_forms_refuse_a_piece_order_x(dev):
    """A piece-order x handed to the row-split form (K1r), to fp32 or split-bf16 math, to the two-launch form, or with x not bf16,
    and parameter pieces on this call, return BNN_ERR_ENUM and launch nothing."""
    S, B, K, N = 3, 128, 64, 10
    x16 = x_of(S, B, K, dev, 5)
    xin = pieces_of(x16, dev)
    w = layer(K, N, 9, dev)

    def refused(x, wts=w, **over):
        with pytest.raises(ops.BnnHipError, match=f"status {ERR_ENUM} "):
            final(x, wts, S, B, K, N, dev, out=out, **over)
    out = torch.zeros((S, B, N), dtype=torch.float32, device=dev)
    refused(xin, wts=(None,) * 4, eps_mode=L.EPS_ZERO, want_stats=False, workspace=None, sample_counter=None, seed=0, layer_id=0,
            sample_offset=0, w_sampled=torch.zeros((S, N, K), dtype=torch.bfloat16, device=dev),
            b_sampled=torch.zeros((S, N), dtype=torch.float32, device=dev), below=(ops.bbb_workspace(S, N, dev), K, N))   # K1r
    refused(xin, math_mode=L.MATH_F32)
    lo = torch.zeros_like(xin)
    lo.bnn_pieces = xin.bnn_pieces
    refused(xin, math_mode=L.MATH_BF16X3, x_lo=lo)
    refused(xin, form=L.FORM_TILE)                                  # the two-launch form
    xf = torch.zeros(tuple(xin.shape), dtype=torch.float32, device=dev)
    xf.bnn_pieces = xin.bnn_pieces
    refused(xf)                                                     # x not bf16
    refused(x16, w_sigma=ops.softplus(w[1]), w_pieces=ops.param_pieces(N, K, dev))
    torch.cuda.synchronize()
    assert not bool(out.view(torch.int32).any())                    # nothing was written
