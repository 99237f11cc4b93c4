"""The prepare launch's piece-order jobs (bnn_eval_prepare; include/bnn_hip.h, bnn_layout and bnn_bbb_fwd_args.w_pieces): the cast
whose blocks stream a 16-row batch tile through LDS, and the parameter-piece jobs beside the row-major sigma of their tensors.
Every assertion is BIT equality, against the same library's row-major path (ops.eval_prepare without cast_out / pieces, ops.softplus)
put through a host re-ordering written out from the layout definitions, which are restated here and not taken from the package:
activations [row][batch block of 128][k-step t][batch tile m][lane][8 bf16], lane (r = lane & 15, q = lane >> 4) of piece (t, m)
holding x[128 block + 16 m + r][32 t + 8 q .. + 7]; parameters [feature tile T][k-step t][mu lo | mu hi | sigma lo | sigma hi][lane]
[4 fp32], lane (r, q) holding mu | sigma [16 T + r][32 t + 8 q + 0..3] (lo) and + 4..7 (hi); both zero-padded, and no launch
writes a pad position."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from bnn_hip import ops


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


def piece_index(shape):
    """int64 [rows, B, K]: the position (in bf16 elements) of every logical element in the piece-order buffer, and its length."""
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


def off4(t):
    """The same values in a tensor that starts 4 bytes into its storage (4-byte aligned only)."""
    base = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = base[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def make_x(shape, seed, dev):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    return ((torch.rand(*shape, generator=gen) - 0.5) * 3.0).to(dev)


def make_param(N, K, seed, dev):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    mu = ((torch.rand((N, K), generator=gen) - 0.5) * 0.4).to(dev)
    rho = (torch.rand((N, K), generator=gen) * 6.0 - 5.0).to(dev)
    return mu, rho


CAST = [((1, 16, 8), False),         # one tile, one chunk
        ((1, 128, 64), False),       # all full
        ((2, 100, 40), False),       # short last tile, 8-k tail
        ((2, 129, 104), False),      # a second batch block of one row, 8-k tail after three full steps
        ((1, 32, 160), False),       # five k-steps, not a multiple of four
        ((3, 128, 784), False),      # the first layer's 16-k tail
        ((130, 72), False),          # 2-D input
        ((1, 20, 1056), False),      # K > 1024: two K chunks, the second a single k-step
        ((2, 100, 40), True)]        # the source starts 4 bytes into its storage: the scalar-load path


@pytest.mark.parametrize("shape,unaligned", CAST)
def test_cast_into_piece_order(dev, shape, unaligned):
    """The whole piece-order buffer, pads included, = the host re-ordering of the row-major cast of the same x."""
    x = make_x(shape, sum(shape) + 7 * len(shape), dev)
    _, c_r, _ = ops.eval_prepare([], cast=x)
    xin = off4(x) if unaligned else x
    buf = ops.pieces_activation(shape, dev)
    _, c_p, _ = ops.eval_prepare([], cast=xin, cast_out=buf)
    assert c_p is buf
    assert torch.equal(bits(buf), to_pieces(c_r))


def test_pads_survive_a_second_launch(dev):
    """Two prepare launches with different x into the same buffer leave it equal to the host re-ordering of the second x."""
    shape = (2, 100, 40)
    buf = ops.pieces_activation(shape, dev)
    for seed in (1, 2):
        x = make_x(shape, seed, dev)
        ops.eval_prepare([], cast=x, cast_out=buf)
    _, c_r, _ = ops.eval_prepare([], cast=x)
    assert torch.equal(bits(buf), to_pieces(c_r))


@pytest.mark.parametrize("N,K", [(16, 8), (72, 40), (80, 784)])
@pytest.mark.parametrize("sigma_unaligned", [False, True])
def test_parameter_pieces_and_row_major_sigma_of_one_launch(dev, N, K, sigma_unaligned):
    """A tensor with pieces: its pieces (pads included) and its row-major sigma equal the row-major launch's and ops.softplus's,
    also into a sigma that is only 4-byte aligned."""
    mu, rho = make_param(N, K, N * 1000 + K, dev)
    sig_r = ops.eval_prepare([rho])[0][0]
    assert torch.equal(bits(sig_r), bits(ops.softplus(rho)))
    wp = ops.param_pieces(N, K, dev)
    sg = torch.full((N, K), -1.0, device=dev)
    sg = off4(sg) if sigma_unaligned else sg
    got = ops.eval_prepare([rho], sigmas=[sg], mus=[mu], pieces=[wp])[0][0]
    assert got is sg
    assert torch.equal(bits(sg), bits(sig_r))
    assert torch.equal(bits(wp), params_to_pieces(mu, sig_r))


def test_tensors_with_and_without_pieces_beside_a_cast(dev):
    """One launch with three tensors -- pieces, none (a 1-D bias rho), pieces -- and a piece-order cast: all three sigmas, both
    piece buffers and the cast are bit-equal to the separate launches' results."""
    shape = (2, 100, 40)
    x = make_x(shape, 11, dev)
    (mu0, rho0), (mu2, rho2) = make_param(72, 40, 3, dev), make_param(24, 72, 4, dev)
    rho1 = (torch.rand(72, generator=torch.Generator(device="cpu").manual_seed(5)) * 6.0 - 5.0).to(dev)
    # the separate launches
    sep_sig, sep_wp = [], []
    for mu, rho in ((mu0, rho0), (mu2, rho2)):
        wp = ops.param_pieces(rho.shape[0], rho.shape[1], dev)
        sep_sig.append(ops.eval_prepare([rho], mus=[mu], pieces=[wp])[0][0])
        sep_wp.append(wp)
        assert torch.equal(bits(sep_sig[-1]), bits(ops.softplus(rho)))
    sep_sig.insert(1, ops.eval_prepare([rho1])[0][0])
    assert torch.equal(bits(sep_sig[1]), bits(ops.softplus(rho1)))
    sep_buf = ops.pieces_activation(shape, dev)
    ops.eval_prepare([], cast=x, cast_out=sep_buf)
    # the one launch
    wp0, wp2, buf = ops.param_pieces(72, 40, dev), ops.param_pieces(24, 72, dev), ops.pieces_activation(shape, dev)
    sig, c, _ = ops.eval_prepare([rho0, rho1, rho2], cast=x, cast_out=buf, mus=[mu0, None, mu2], pieces=[wp0, None, wp2])
    assert c is buf
    for got, want in zip(sig, sep_sig):
        assert got.shape == want.shape and torch.equal(bits(got), bits(want))
    assert torch.equal(bits(wp0), bits(sep_wp[0])) and torch.equal(bits(wp2), bits(sep_wp[1]))
    assert torch.equal(bits(wp0), params_to_pieces(mu0, sep_sig[0])) and torch.equal(bits(wp2), params_to_pieces(mu2, sep_sig[2]))
    assert torch.equal(bits(buf), bits(sep_buf))
    assert torch.equal(bits(buf), to_pieces(ops.eval_prepare([], cast=x)[1]))
