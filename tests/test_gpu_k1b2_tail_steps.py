"""The last steps of a piece-order launch of the pair block GEMM K1b2 (csrc/bbb_linear.hip, `step`'s LAST forms): with x and the
parameters in piece order a wave with a full feature tile runs EVERY step on its straight-line body -- the last whole step in the
maskless loop, then one last-step form: whole (K % 32 == 0), the K tail without weight masks (the pads are zeros in memory), or
the K tail with the half-width generator (tail <= 16 k: lanes 32 .. 63 draw the second Philox group of lanes 0 .. 31 and hand the
normals down with v_permlane32_swap_b32).  The reference is the SAME launch with the layouts off (row-major x, no `w_pieces`),
which runs the generic masked steps as before; every comparison is BIT equality: y, and the per-tile statistics workspace
(header, then per (sample, feature tile) the sums of eps^2, of w^2 and -- sample 0 -- of log sigma).

Shapes (S = 4 pairs; form forced to the block GEMM with a hoisted sigma, `waves == 8` asserted from the plan):
  K = 64 no tail (the whole last-step form), 80 tail of 16 (half-width generator), 72 tail of 8 (three quarters of the lanes
  padded), 88 tail of 24 (full-width generator in the tail form), 32 one step and no loop, 48 one whole step + a tail of 16;
  N = 64 (full tiles), 80 (a phantom wave in the last feature group), 72 (a partial last tile: that wave keeps the generic step);
  batch 128, and 40 for the row edge in the epilogue.
`want_stats` on and off covers bodies 1 .. 3 (sample 0 takes the body with the log sigma sum); a mixture prior keeps the generic
path and is unchanged.  The piece-order index maps are restated in tools/k1b2_step_forms.py from include/bnn_hip.h."""
import os
import sys

import pytest
import torch

import bnn_hip
from bnn_hip import _lib as L
from bnn_hip import ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import k1b2_step_forms as SF          # noqa: E402  (to_pieces / params_to_pieces: the host re-ordering)

pytestmark = pytest.mark.gpu

S = 4
# (K, N, B)
SHAPES = [(64, 64, 128), (64, 80, 128),
          (80, 64, 128), (80, 80, 128), (80, 64, 40), (80, 80, 40),
          (72, 64, 128), (72, 80, 128),
          (88, 64, 128), (88, 80, 128),
          (32, 64, 128), (32, 80, 128),
          (48, 64, 128), (48, 80, 128),
          (80, 72, 128)]               # a partial last feature tile: its wave stays generic beside the straight-line ones
GAUSS, MIXTURE = ops.PriorSpec(False, 0.9), ops.PriorSpec(True, 1.0, 0.5, 1.0, 0.05)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _bf16_math():
    bnn_hip.set_math("bf16")
    yield
    bnn_hip.set_math("bf16")


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).reshape(-1)


_cache = {}


def operands(shape, dev):
    """Per shape, made once: row-major x, its piece-order copy, the layer, the hoisted sigma, (mu, sigma) in piece order."""
    if shape not in _cache:
        K, N, B = shape
        gen = torch.Generator(device="cpu").manual_seed(K * 1000 + N * 7 + B)
        x = (torch.rand(S, B, K, generator=gen) - 0.3).to(torch.bfloat16)
        wm = (torch.rand((N, K), generator=gen) - 0.5) * 0.4
        wr = torch.rand((N, K), generator=gen) - 5.0
        bm = (torch.rand(N, generator=gen) - 0.5) * 0.4
        br = torch.rand(N, generator=gen) - 5.0
        sig = ops.softplus(wr.to(dev))
        xp = ops.pieces_activation((S, B, K), dev)
        xp.view(torch.int16).view(-1).copy_(SF.to_pieces(x).to(dev))
        wp = ops.param_pieces(N, K, dev)
        wp.view(torch.int32).view(-1).copy_(SF.params_to_pieces(wm, sig).to(dev))
        _cache[shape] = (x.to(dev), xp, tuple(a.to(dev) for a in (wm, wr, bm, br)), sig, wp)
    return _cache[shape]


def launch(shape, dev, pieces, want_stats, prior=GAUSS, y_pieces=False):
    """One forced K1b2 launch; returns (y row-major, the statistics workspace's written words or None)."""
    K, N, B = shape
    x, xp, w, sig, wp = operands(shape, dev)
    kw = dict(n_samples=S, prior=prior, math_mode=L.MATH_BF16, relu=True, y_dtype=torch.bfloat16, eps_mode=L.EPS_PHILOX,
              seed=41, layer_id=1, sample_offset=3, want_stats=want_stats, want_scalars=False, dump_eps=False,
              form=L.FORM_GEMM, w_sigma=sig)
    if pieces:
        kw.update(w_pieces=wp)
        if y_pieces:
            kw.update(out=ops.pieces_activation((S, B, N), dev))
    xin = xp if pieces else x
    plan = ops.bbb_plan(xin, *w, **kw)
    assert plan["form"] == L.FORM_GEMM and plan["waves"] == 8, plan
    out = ops.bbb_linear_fwd(xin, *w, **kw)
    torch.cuda.synchronize()
    y = ops.unpiece(out["y"]) if (pieces and y_pieces) else out["y"]
    ws = None
    if want_stats:
        T = (N + 15) // 16
        ws = out["workspace"][:4 * (1 + S * T)].clone()          # float4 header + one float4 per (sample, feature tile)
    return y, ws


@pytest.fixture(scope="module")
def reference(dev):
    """Per (shape, want_stats, prior kind): the row-major launch's results (computed on first use, never modified)."""
    res = {}

    def get(shape, want_stats, prior=GAUSS):
        key = (shape, want_stats, prior.mixture)
        if key not in res:
            res[key] = launch(shape, dev, False, want_stats, prior)
        return res[key]
    return get


def check(got, ref):
    assert torch.equal(bits(got[0]), bits(ref[0])), "y"
    if ref[1] is not None:
        assert torch.equal(bits(got[1]), bits(ref[1])), "statistics workspace"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "K%d-N%d-B%d" % s)
@pytest.mark.parametrize("want_stats", [True, False])
def test_piece_order_last_steps_equal_the_generic_steps(dev, reference, shape, want_stats):
    """x and the parameters in piece order (every step of a full-tile wave on its straight-line body) = the row-major launch (the
    generic masked last steps): y and the statistics workspace bit for bit."""
    check(launch(shape, dev, True, want_stats), reference(shape, want_stats))


@pytest.mark.parametrize("shape", [(64, 64, 128), (80, 80, 40), (72, 64, 128), (88, 80, 128), (48, 64, 128)],
                         ids=lambda s: "K%d-N%d-B%d" % s)
def test_with_a_piece_order_y(dev, reference, shape):
    """The same with y written in piece order too (the form the headline's layers launch)."""
    check(launch(shape, dev, True, True, y_pieces=True), reference(shape, True))


@pytest.mark.parametrize("shape", [(80, 80, 128), (64, 64, 128)], ids=lambda s: "K%d-N%d-B%d" % s)
def test_mixture_prior_keeps_the_generic_steps(dev, reference, shape):
    """A mixture prior takes no straight-line body: piece-order and row-major launches agree as before."""
    check(launch(shape, dev, True, True, prior=MIXTURE), reference(shape, True, MIXTURE))


def test_two_piece_order_launches_give_identical_bits(dev):
    a = launch((80, 80, 128), dev, True, True)
    b = launch((80, 80, 128), dev, True, True)
    check(a, b)
