"""Thin tensor-level wrappers over the C ABI.  torch is used only for device memory and
the current HIP stream; every operation here is one or two kernels of libbnn_hip.so."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import NamedTuple, Optional, Sequence

import torch

from . import _lib as L
from ._lib import BnnHipError


@dataclass(frozen=True)
class PriorSpec:
    """Prior of a layer: Gaussian N(0, sigma_p) or the scale mixture of networks.py:14-27."""
    mixture: bool = False
    sigma_p: float = 1.0
    pi: float = 0.5
    sigma1: float = 1.0
    sigma2: float = 1.0

    @staticmethod
    def from_init(prior_init: Sequence[float], mixture: bool) -> "PriorSpec":
        if mixture:
            assert len(prior_init) == 3, "Scale Mixture Prior requires three values in prior initialisation"
            return PriorSpec(True, 1.0, float(prior_init[0]), math.exp(prior_init[1]), math.exp(prior_init[2]))
        assert len(prior_init) == 1, "Gaussian Prior requires one value in prior initialisation"
        return PriorSpec(False, float(prior_init[0]))

    def c(self) -> L.Prior:
        return L.Prior(L.PRIOR_MIXTURE if self.mixture else L.PRIOR_GAUSS, self.sigma_p, self.pi,
                       self.sigma1, self.sigma2)


def _stream() -> int:
    """Raw hipStream_t of the current stream of the current device.  (torch.cuda.current_stream() without a
    device walks through is_available() and an os.getenv on every call: ~20-60 us, more than a launch.)"""
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())


def require_device(*tensors: torch.Tensor):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise BnnHipError(
                "bnn_hip: the Bayes-by-backprop hot path runs on a ROCm device only (tensor is on "
                f"{t.device}); there is no CPU fallback.  Move the module and its inputs to DEVICE.")


def _f32c(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise BnnHipError(f"{name} must be float32, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return L.F32
    if t.dtype == torch.bfloat16:
        return L.BF16
    raise BnnHipError(f"activations must be float32 or bfloat16, got {t.dtype}")


def _exact_unless_bf16(math_mode: int) -> int:
    """The split-bf16 mode (MATH_BF16X3) exists for the BBB forward kernels; every other launch of a job in that mode --
    the local-reparameterisation layers, the backward kernels -- runs the exact-fp32 matrix core."""
    return L.MATH_F32 if math_mode == L.MATH_BF16X3 else math_mode


def pieces_activation(shape, device) -> torch.Tensor:
    """A zeroed bf16 activation buffer in PIECE ORDER (include/bnn_hip.h, bnn_layout) for the logical tensor `shape` =
    [batch, features] or [rows, batch, features]: [rows * ceil(batch / 128)][ceil(features / 32)][8 batch tiles][64 lanes][8].
    The layout travels with the tensor OBJECT (its `bnn_pieces` attribute holds the logical shape): bbb_linear_fwd / bbb_plan /
    bbb_final_fwd (its x, where the output layer runs as one launch) / eval_prepare read it from the `x`, `out` and `cast_out` they
    are handed, every other entry point refuses such a tensor.
    Pad positions are never written by a launch, so the buffer is zeroed once, here."""
    shape = tuple(int(d) for d in shape)
    if len(shape) not in (2, 3) or min(shape) < 1:
        raise BnnHipError(f"pieces_activation: shape must be [batch,features] or [rows,batch,features], got {shape}")
    rows = shape[0] if len(shape) == 3 else 1
    t = torch.zeros((rows * ((shape[-2] + 127) // 128), (shape[-1] + 31) // 32, 8, 64, 8), dtype=torch.bfloat16, device=device)
    t.bnn_pieces = shape
    return t


def param_pieces(out_features: int, in_features: int, device) -> torch.Tensor:
    """A zeroed buffer for the (mu, sigma) of one [out, in] layer in the piece order of the pair block GEMM (include/bnn_hip.h,
    bnn_bbb_fwd_args.w_pieces): fp32 [feature tiles][k-steps][mu lo | mu hi | sigma lo | sigma hi][64 lanes][4].  eval_prepare
    (`mus`, `pieces`) fills it from the current parameters; bbb_linear_fwd / bbb_plan take it as `w_pieces`, or find it as the
    `bnn_param_pieces` attribute of the `w_sigma` tensor they are handed."""
    return torch.zeros(((out_features + 15) // 16, (in_features + 31) // 32, 4, 64, 4), dtype=torch.float32, device=device)


def pieces_shape(t: Optional[torch.Tensor]):
    """The logical shape of a piece-order activation buffer, None for a row-major tensor."""
    return getattr(t, "bnn_pieces", None) if t is not None else None


def unpiece(t: torch.Tensor) -> torch.Tensor:
    """The row-major copy of a piece-order activation buffer (its logical shape)."""
    shape = pieces_shape(t)
    rows, B, K = (shape if len(shape) == 3 else (1,) + shape)
    mbs, ks = (B + 127) // 128, (K + 31) // 32
    # [row, mb, t, m, q, r, 8] -> [row, mb, m, r, t, q, 8]
    v = t.view(rows, mbs, ks, 8, 4, 16, 8).permute(0, 1, 3, 5, 2, 4, 6).reshape(rows, mbs * 128, ks * 32)
    return v[:, :B, :K].reshape(shape).contiguous()


def _x3(x: torch.Tensor, n_samples: int, pieces_ok: bool = False):
    """Returns (contiguous x, batch, in_features, x_per_sample): 0 = one x for all samples, g >= 1 = sample s reads
    x[s // g] (x [rows, batch, in] with rows * g == n_samples: g = 1 is one x per sample, g = S is one x per minibatch
    of S MC samples).  A piece-order x (pieces_activation) counts by its logical shape, where the caller can pass the layout on."""
    shape = pieces_shape(x)
    if shape is not None:
        if not pieces_ok:
            raise BnnHipError("a piece-order activation buffer (ops.pieces_activation) is read by bbb_linear_fwd / bbb_final_fwd only")
        if len(shape) == 3 and n_samples % shape[0]:
            raise BnnHipError(f"x has {shape[0]} row blocks, which does not divide {n_samples} samples")
        return x, shape[-2], shape[-1], (n_samples // shape[0] if len(shape) == 3 else 0)
    if x.dim() == 2:
        xs = x if x.is_contiguous() else x.contiguous()
        return xs, x.shape[0], x.shape[1], 0
    if x.dim() == 3:
        if x.shape[0] < 1 or n_samples % x.shape[0]:
            raise BnnHipError(f"x has {x.shape[0]} row blocks, which does not divide {n_samples} samples")
        xs = x if x.is_contiguous() else x.contiguous()
        return xs, x.shape[1], x.shape[2], n_samples // x.shape[0]
    raise BnnHipError(f"x must be [batch,in] or [rows,batch,in], got {tuple(x.shape)}")


def bbb_workspace(n_samples: int, out_features: int, device) -> torch.Tensor:
    nbytes = L.load().bnn_bbb_linear_fwd_workspace_bytes(n_samples, out_features)
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device)


def split_scratch(n_samples: int, batch: int, out_features: int, device) -> torch.Tensor:
    """Scratch for the K-sliced GEMM form of K1: arrival counters (zeroed here, once; launches leave them zero) followed
    by the fp32 partial tiles (uninitialised).  One scratch serves one launch at a time."""
    lib = L.load()
    nbytes = lib.bnn_bbb_split_scratch_bytes(n_samples, batch, out_features)
    t = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=device)
    t[:lib.bnn_bbb_split_scratch_zero_bytes(n_samples, batch, out_features) // 4].zero_()
    return t


_split_cache = {}


def split_scratch_cached(n_samples: int, batch: int, out_features: int, device) -> torch.Tensor:
    """The eager path's scratch: one per (device, current stream, shape), allocated and zeroed once -- launches on one
    stream run one after the other and each leaves the counters at zero.  (Captured evaluators own theirs.)"""
    if torch.cuda.is_current_stream_capturing():
        return split_scratch(n_samples, batch, out_features, device)
    key = (str(device), torch.cuda.current_stream(device).cuda_stream, n_samples, batch, out_features)
    t = _split_cache.get(key)
    if t is None:
        if len(_split_cache) >= 16:
            _split_cache.clear()
        t = _split_cache[key] = split_scratch(n_samples, batch, out_features, device)
    return t


def final_scratch(n_samples: int, device) -> torch.Tensor:
    """Zeroed scratch for the fused last layer (K-range slices per sample)."""
    nbytes = L.load().bnn_bbb_final_scratch_bytes(n_samples)
    return torch.zeros((nbytes + 3) // 4, dtype=torch.int32, device=device)


def lr_split_scratch(n_samples: int, batch: int, out_features: int, device) -> torch.Tensor:
    """Scratch for the K-sliced form of K3 (1-3 samples on a wide LR layer): arrival counters (zeroed here, once; launches
    leave them zero) followed by the fp32 partial tiles.  One scratch serves one launch at a time."""
    lib = L.load()
    nbytes = lib.bnn_lr_split_scratch_bytes(n_samples, batch, out_features)
    t = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=device)
    t[:lib.bnn_lr_split_scratch_zero_bytes(n_samples, batch, out_features) // 4].zero_()
    return t


_lr_split_cache = {}


def lr_split_scratch_cached(n_samples: int, batch: int, out_features: int, device) -> torch.Tensor:
    """The eager path's K3s scratch: one per (device, current stream, shape), as split_scratch_cached."""
    if torch.cuda.is_current_stream_capturing():
        return lr_split_scratch(n_samples, batch, out_features, device)
    key = (str(device), torch.cuda.current_stream(device).cuda_stream, n_samples, batch, out_features)
    t = _lr_split_cache.get(key)
    if t is None:
        if len(_lr_split_cache) >= 16:
            _lr_split_cache.clear()
        t = _lr_split_cache[key] = lr_split_scratch(n_samples, batch, out_features, device)
    return t


def lr_workspace(out_features: int, device) -> torch.Tensor:
    nbytes = L.load().bnn_lr_linear_fwd_workspace_bytes(out_features)
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device)


def _y16(a, y: torch.Tensor) -> torch.Tensor:
    """y_bf16_copy of a layer call: fp32 y for the backward, bf16 y for the next layer's forward (tile forms)."""
    if y.dtype != torch.float32:
        raise BnnHipError("want_y16 goes with fp32 y")
    y16 = torch.empty(tuple(y.shape), dtype=torch.bfloat16, device=y.device)
    a.y_bf16_copy = y16.data_ptr()
    return y16


def _layouts(x, y, n_samples: int, B: int, N: int):
    """(x_layout, y_layout) of a K1 call from the tensors themselves (ops.pieces_activation marks a buffer)."""
    ys = pieces_shape(y)
    if ys is not None and tuple(ys) != (n_samples, B, N):
        raise BnnHipError(f"out: a piece-order buffer for {tuple(ys)}, the launch writes {(n_samples, B, N)}")
    return (L.LAYOUT_PIECES if pieces_shape(x) is not None else L.LAYOUT_ROWS,
            L.LAYOUT_PIECES if ys is not None else L.LAYOUT_ROWS)


def _bbb_build(x, w_mu, w_rho, b_mu, b_rho, *, n_samples: int, prior: PriorSpec, math_mode: int,
               relu: bool, y_dtype: torch.dtype, eps_mode: int, eps_w=None, eps_b=None, seed: int = 0,
               layer_id: int = 0, sample_offset: int = 0, want_stats: bool = True,
               want_scalars: bool = False, dump_eps: bool = False, workspace=None, sample_counter=None,
               out=None, split_scratch=None, w_sigma=None, form: int = 0, sample_group: int = 0,
               sample_group_stride: int = 0, w_sampled=None, b_sampled=None, rider=None, want_y16: bool = False, wt_out=None,
               x_lo=None, out_lo=None, w_pieces=None):
    """Argument block of K1 + the tensors it points at (kept alive by the caller).  `w_sampled` / `b_sampled` (bf16
    [S,out,in] / fp32 [S,out] from bbb_sample_weights): the matmul-only form, the parameter tensors may then be None.
    `rider` = the (args, results, keep) of build_sample_job: an independent sampling job carried by the launch."""
    require_device(x, w_mu, w_rho, b_mu, b_rho, eps_w, eps_b, w_sampled, b_sampled)
    if w_sampled is not None:
        if w_sampled.dtype != torch.bfloat16 or b_sampled is None or b_sampled.dtype != torch.float32 or \
                not w_sampled.is_contiguous() or not b_sampled.is_contiguous() or w_sampled.dim() != 3:
            raise BnnHipError("w_sampled must be contiguous bf16 [S,out,in], b_sampled contiguous fp32 [S,out]")
        if w_sampled.shape[0] != n_samples or b_sampled.numel() != n_samples * w_sampled.shape[1]:
            raise BnnHipError("w_sampled / b_sampled do not match n_samples")
        N, K = w_sampled.shape[1], w_sampled.shape[2]
        xs, B, Kx, per_sample = _x3(x, n_samples, pieces_ok=True)
        if Kx != K:
            raise BnnHipError(f"shape mismatch: x[...,{Kx}] sampled weight {tuple(w_sampled.shape)}")
        y = out if out is not None else torch.empty((n_samples, B, N), dtype=y_dtype, device=xs.device)
        a = L.BbbFwdArgs()
        a.struct_bytes = C.sizeof(L.BbbFwdArgs)
        a.n_samples, a.batch, a.in_features, a.out_features = n_samples, B, K, N
        a.x, a.x_dtype, a.x_per_sample = xs.data_ptr(), _dt(xs), per_sample
        a.x_layout, a.y_layout = _layouts(xs, y, n_samples, B, N)      # (the library refuses them for this form)
        a.eps_mode, a.math = L.EPS_ZERO, L.MATH_BF16
        a.want_stats, a.relu = 0, int(relu)
        a.y, a.y_dtype = y.data_ptr(), _dt(y)
        a.w_sampled, a.b_sampled = w_sampled.data_ptr(), b_sampled.data_ptr()
        if wt_out is not None:                       # the same weights once more, transposed (for the layer's input gradient)
            require_device(wt_out)
            if wt_out.dtype != torch.bfloat16 or not wt_out.is_contiguous() or tuple(wt_out.shape) != (n_samples, K, N):
                raise BnnHipError("wt_out must be a contiguous bf16 [samples,in,out] tensor")
            a.w_sampled_t_out = wt_out.data_ptr()
        a.form = int(form)
        y16 = _y16(a, y) if want_y16 else None
        return a, dict(y=y, y16=y16, workspace=None, log_prior=None, log_q=None, eps_w=None, eps_b=None), (xs, w_sampled, b_sampled, y)
    w_mu, w_rho = _f32c(w_mu, "weight_mu"), _f32c(w_rho, "weight_rho")
    b_mu, b_rho = _f32c(b_mu, "bias_mu"), _f32c(b_rho, "bias_rho")
    N, K = w_mu.shape
    xs, B, Kx, per_sample = _x3(x, n_samples, pieces_ok=True)
    if Kx != K or tuple(w_rho.shape) != (N, K) or tuple(b_mu.shape) != (N,) or tuple(b_rho.shape) != (N,):
        raise BnnHipError(f"shape mismatch: x[...,{Kx}] weight {tuple(w_mu.shape)} bias {tuple(b_mu.shape)}")
    dev = xs.device
    y = out if out is not None else torch.empty((n_samples, B, N), dtype=y_dtype, device=dev)
    if want_stats and workspace is None:
        workspace = bbb_workspace(n_samples, N, dev)
    lp = torch.empty(n_samples, dtype=torch.float32, device=dev) if want_scalars else None
    lq = torch.empty(n_samples, dtype=torch.float32, device=dev) if want_scalars else None
    if eps_mode == L.EPS_MEMORY:
        eps_w, eps_b = _f32c(eps_w, "eps_w"), _f32c(eps_b, "eps_b")
        if eps_w.numel() != n_samples * N * K or eps_b.numel() != n_samples * N:
            raise BnnHipError("eps_w/eps_b must be [samples,out,in] / [samples,out]")
    dw = torch.empty((n_samples, N, K), dtype=torch.float32, device=dev) if dump_eps else None
    db = torch.empty((n_samples, N), dtype=torch.float32, device=dev) if dump_eps else None
    a = L.BbbFwdArgs()
    a.struct_bytes = C.sizeof(L.BbbFwdArgs)
    a.n_samples, a.batch, a.in_features, a.out_features = n_samples, B, K, N
    a.x, a.x_dtype, a.x_per_sample = xs.data_ptr(), _dt(xs), per_sample
    a.w_mu, a.w_rho, a.b_mu, a.b_rho = w_mu.data_ptr(), w_rho.data_ptr(), b_mu.data_ptr(), b_rho.data_ptr()
    a.eps_mode, a.math = eps_mode, math_mode
    a.eps_w, a.eps_b = _ptr(eps_w) if eps_mode == L.EPS_MEMORY else None, _ptr(eps_b) if eps_mode == L.EPS_MEMORY else None
    a.seed, a.layer_id, a.sample_offset = seed & 0xFFFFFFFFFFFFFFFF, layer_id, sample_offset & 0xFFFFFFFF
    a.sample_counter = _ptr(sample_counter)
    a.sample_group, a.sample_group_stride = int(sample_group), int(sample_group_stride)
    a.form = int(form)
    a.eps_w_dump, a.eps_b_dump = _ptr(dw), _ptr(db)
    a.prior = prior.c()
    a.want_stats, a.relu = int(want_stats), int(relu)
    a.workspace = _ptr(workspace) if want_stats else None
    a.workspace_bytes = workspace.numel() * 4 if (want_stats and workspace is not None) else 0
    a.log_prior, a.log_q = _ptr(lp), _ptr(lq)
    a.y, a.y_dtype = y.data_ptr(), _dt(y)
    a.x_layout, a.y_layout = _layouts(xs, y, n_samples, B, N)
    y_lo = None
    if math_mode == L.MATH_BF16X3:
        # split-bf16 math: a bf16 activation is a PAIR of planes (hi = x / y, lo = x_lo / out_lo), fp32 ones are split on chip
        if xs.dtype == torch.bfloat16:
            if x_lo is None or x_lo.dtype != torch.bfloat16 or tuple(x_lo.shape) != tuple(x.shape) or not x_lo.is_contiguous():
                raise BnnHipError("bf16x3 math on bf16 x needs x_lo: the contiguous bf16 low plane, shaped like x")
            require_device(x_lo)
            a.x_lo = x_lo.data_ptr()
        if y.dtype == torch.bfloat16:
            y_lo = out_lo if out_lo is not None else torch.empty(tuple(y.shape), dtype=torch.bfloat16, device=dev)
            if y_lo.dtype != torch.bfloat16 or y_lo.numel() != y.numel() or not y_lo.is_contiguous():
                raise BnnHipError("out_lo must be a contiguous bf16 tensor shaped like y")
            a.y_lo = y_lo.data_ptr()
    if w_sigma is not None:
        a.w_sigma = w_sigma.data_ptr()
        if w_pieces is None:
            w_pieces = getattr(w_sigma, "bnn_param_pieces", None)
    if w_pieces is not None:
        require_device(w_pieces)
        if w_sigma is None or w_pieces.dtype != torch.float32 or not w_pieces.is_contiguous() or \
                w_pieces.numel() != ((N + 15) // 16) * ((K + 31) // 32) * 1024:
            raise BnnHipError("w_pieces: ops.param_pieces(out, in) filled by eval_prepare, beside w_sigma")
        a.w_pieces = w_pieces.data_ptr()
    if split_scratch is not None:
        a.split_scratch = split_scratch.data_ptr()
        a.split_scratch_bytes = split_scratch.numel() * split_scratch.element_size()
    if rider is not None:
        a.rider = C.addressof(rider[0])
    res = dict(y=y, y16=_y16(a, y) if want_y16 else None, workspace=workspace, log_prior=lp, log_q=lq, eps_w=dw, eps_b=db, y_lo=y_lo)
    keep = (xs, w_mu, w_rho, b_mu, b_rho, eps_w, eps_b, sample_counter, split_scratch, w_sigma, rider, x_lo, y_lo, w_pieces)
    a._keep = keep                    # (the structure owns what its pointers refer to: engine.GraphedElbo(capture="calls") replays it)
    return a, res, keep


def bbb_linear_fwd(x, w_mu, w_rho, b_mu, b_rho, **kw):
    """K1.  Returns dict(y, workspace, log_prior, log_q, eps_w, eps_b)."""
    lib = L.load()
    a, res, keep = _bbb_build(x, w_mu, w_rho, b_mu, b_rho, **kw)
    L.check(lib.bnn_bbb_linear_fwd(C.byref(a), _stream()), "bnn_bbb_linear_fwd")
    return res


def _plan_dict(pl: L.Plan) -> dict:
    return {k: getattr(pl, k) for k, _ in L.Plan._fields_}


def bbb_plan(x, w_mu, w_rho, b_mu, b_rho, **kw) -> dict:
    """bnn_bbb_plan: the launch geometry bbb_linear_fwd would use for these arguments (no launch)."""
    a, res, keep = _bbb_build(x, w_mu, w_rho, b_mu, b_rho, **kw)
    pl = L.Plan()
    L.check(L.load().bnn_bbb_plan(C.byref(a), C.byref(pl)), "bnn_bbb_plan")
    return _plan_dict(pl)


def sample_workspace(n_samples: int, fin: int, fout: int, device) -> torch.Tensor:
    """Statistics workspace of one layer that serves both K1 (fused) and K1s (split) forms."""
    nbytes = L.load().bnn_bbb_sample_workspace_bytes(n_samples, fin, fout) or \
        L.load().bnn_bbb_linear_fwd_workspace_bytes(n_samples, fout)
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device)


def build_sample_job(layers, *, n_samples: int, seed: int = 0, sample_offset: int = 0, sample_counter=None, cast=None,
                     sample_group: int = 0, sample_group_stride: int = 0):
    """Argument block of K1s (bnn_bbb_sample_weights) + its results + the tensors it points at: launched by
    bbb_sample_weights, or handed to a layer launch as its `rider`.  `layers` = list of dicts(w_mu [out,in], w_rho,
    b_mu, b_rho, prior, layer_id, workspace=None, w_out=None, b_out=None); results = list of dicts(w [S,out,in] bf16,
    b [S,out] fp32, workspace).  `cast` = (fp32 tensor, bf16 tensor): also converts the input batch in that launch."""
    if not 1 <= len(layers) <= L.SAMPLE_MAX_LAYERS:
        raise BnnHipError(f"bbb_sample_weights: 1..{L.SAMPLE_MAX_LAYERS} layers per launch")
    a = L.SampleArgs()
    a.struct_bytes = C.sizeof(L.SampleArgs)
    a.n_layers, a.n_samples = len(layers), int(n_samples)
    a.seed, a.sample_offset = seed & 0xFFFFFFFFFFFFFFFF, sample_offset & 0xFFFFFFFF
    a.sample_counter = _ptr(sample_counter)
    a.sample_group, a.sample_group_stride = int(sample_group), int(sample_group_stride)
    res, keep = [], [sample_counter]
    for i, ly in enumerate(layers):
        w_mu, w_rho = _f32c(ly["w_mu"], "weight_mu"), _f32c(ly["w_rho"], "weight_rho")
        b_mu, b_rho = _f32c(ly["b_mu"], "bias_mu"), _f32c(ly["b_rho"], "bias_rho")
        require_device(w_mu, w_rho, b_mu, b_rho)
        N, K = w_mu.shape
        if K % 8:
            raise BnnHipError("bbb_sample_weights: in_features must be a multiple of 8")
        if tuple(w_rho.shape) != (N, K) or tuple(b_mu.shape) != (N,) or tuple(b_rho.shape) != (N,):
            raise BnnHipError("bbb_sample_weights: parameter shapes disagree")
        dev = w_mu.device
        ws = ly.get("workspace")
        if ws is None:
            ws = sample_workspace(n_samples, K, N, dev)
        w = ly.get("w_out")
        if w is None:
            w = torch.empty((n_samples, N, K), dtype=torch.bfloat16, device=dev)
        b = ly.get("b_out")
        if b is None:
            b = torch.empty((n_samples, N), dtype=torch.float32, device=dev)
        if w.dtype != torch.bfloat16 or w.numel() != n_samples * N * K or b.dtype != torch.float32 or b.numel() != n_samples * N:
            raise BnnHipError("bbb_sample_weights: w_out must be bf16 [S,out,in], b_out fp32 [S,out]")
        e = a.layer[i]
        e.in_features, e.out_features, e.layer_id = K, N, int(ly.get("layer_id", i))
        e.w_mu, e.w_rho, e.b_mu, e.b_rho = w_mu.data_ptr(), w_rho.data_ptr(), b_mu.data_ptr(), b_rho.data_ptr()
        e.w_out, e.b_out = w.data_ptr(), b.data_ptr()
        e.workspace, e.workspace_bytes = ws.data_ptr(), ws.numel() * 4
        e.prior = ly["prior"].c()
        res.append(dict(w=w, b=b, workspace=ws))
        keep.append((w_mu, w_rho, b_mu, b_rho, w, b, ws))
    if cast is not None:                      # (fp32 src, bf16 dst): the input batch cast rides on the launch
        src, dst = cast
        require_device(src, dst)
        if src.dtype != torch.float32 or dst.dtype != torch.bfloat16 or src.numel() != dst.numel() or \
                not src.is_contiguous() or not dst.is_contiguous():
            raise BnnHipError("bbb_sample_weights: cast = (contiguous fp32 source, contiguous bf16 destination) of one size")
        a.cast_src, a.cast_dst, a.cast_n = src.data_ptr(), dst.data_ptr(), src.numel()
        keep.append((src, dst))
    a._keep = keep                    # (the structure owns what its pointers refer to: engine.GraphedElbo(capture="calls") replays it)
    return a, res, keep


def bbb_sample_weights(layers, **kw):
    """K1s (bnn_bbb_sample_weights): one launch samples every layer of `layers`; see build_sample_job."""
    a, res, keep = build_sample_job(layers, **kw)
    L.check(L.load().bnn_bbb_sample_weights(C.byref(a), _stream()), "bnn_bbb_sample_weights")
    return res


def bbb_sampled_matmul(x, w, b, *, n_samples: int, relu: bool, y_dtype: torch.dtype, out=None, want_y16: bool = False, wt_out=None,
                       form: int = 0):
    """Matmul half of K1 over weights sampled by bbb_sample_weights: y[s] = act(x[s] . w[s]^T + b[s]).  `want_y16`:
    returns (y fp32, y in bf16).  `wt_out` (bf16 [S,in,out]): the launch also leaves w transposed there."""
    a, res, keep = _bbb_build(x, None, None, None, None, n_samples=n_samples, prior=PriorSpec(), math_mode=L.MATH_BF16, relu=relu,
                              y_dtype=y_dtype, eps_mode=L.EPS_ZERO, want_stats=False, out=out, w_sampled=w, b_sampled=b,
                              want_y16=want_y16, wt_out=wt_out, form=form)
    L.check(L.load().bnn_bbb_linear_fwd(C.byref(a), _stream()), "bnn_bbb_linear_fwd")
    return (res["y"], res["y16"]) if want_y16 else res["y"]


def _lr_build(x, w_mu, w_rho, b_mu, b_rho, *, n_samples: int, sigma_p: float, math_mode: int, relu: bool,
                  y_dtype: torch.dtype, eps_mode: int, eps_act=None, eps_b=None, seed: int = 0, layer_id: int = 0,
                  sample_offset: int = 0, want_kl: bool = True, want_scalars: bool = False,
                  dump_eps: bool = False, workspace=None, sample_counter=None, out=None, x_sq=None,
                  out_sq=None, w_frag=None, want_v: bool = False, want_y16: bool = False, want_hfac: bool = False, form: int = 0,
                  sample_group: int = 0,
                  sample_group_stride: int = 0, split_scratch=None, rider=None, x_lo=None, out_lo=None):
    """Argument block of K3 + the result dict + the tensors it points at.  `rider`: dict(w_mu, w_rho, b_mu, b_rho, w_frag,
    workspace) of a narrow LR layer whose operands this launch prepares on the side (bnn_lr_rider).
    math_mode MATH_BF16X3 (the block form over lr_prepare(x3=True) fragments, bf16 x with `x_lo` and `x_sq`): taken as asked when
    those operands are there, else the launch runs exact fp32 (the mode's promise is the reference's arithmetic)."""
    require_device(x, w_mu, w_rho, b_mu, b_rho, eps_act, eps_b)
    if math_mode == L.MATH_BF16X3 and (x_lo is None or x_sq is None or w_frag is None or x.dtype != torch.bfloat16):
        math_mode = L.MATH_F32
    w_mu, w_rho = _f32c(w_mu, "weight_mu"), _f32c(w_rho, "weight_rho")
    b_mu, b_rho = _f32c(b_mu, "bias_mu"), _f32c(b_rho, "bias_rho")
    K, N = w_mu.shape
    xs, B, Kx, per_sample = _x3(x, n_samples)
    if Kx != K or tuple(w_rho.shape) != (K, N) or tuple(b_mu.shape) != (N,) or tuple(b_rho.shape) != (N,):
        raise BnnHipError(f"shape mismatch: x[...,{Kx}] weight {tuple(w_mu.shape)} bias {tuple(b_mu.shape)}")
    dev = xs.device
    y = out if out is not None else torch.empty((n_samples, B, N), dtype=y_dtype, device=dev)
    if want_kl and workspace is None:
        workspace = lr_workspace(N, dev)
    kl3 = torch.empty(3, dtype=torch.float32, device=dev) if want_scalars else None
    if eps_mode == L.EPS_MEMORY:
        eps_act, eps_b = _f32c(eps_act, "eps_act"), _f32c(eps_b, "eps_b")
        if eps_act.numel() != n_samples * B * N or eps_b.numel() != n_samples * N:
            raise BnnHipError("eps_act/eps_b must be [samples,batch,out] / [samples,out]")
    da = torch.empty((n_samples, B, N), dtype=torch.float32, device=dev) if dump_eps else None
    db = torch.empty((n_samples, N), dtype=torch.float32, device=dev) if dump_eps else None
    a = L.LrFwdArgs()
    a.struct_bytes = C.sizeof(L.LrFwdArgs)
    a.n_samples, a.batch, a.in_features, a.out_features = n_samples, B, K, N
    a.x, a.x_dtype, a.x_per_sample = xs.data_ptr(), _dt(xs), per_sample
    a.w_mu, a.w_rho, a.b_mu, a.b_rho = w_mu.data_ptr(), w_rho.data_ptr(), b_mu.data_ptr(), b_rho.data_ptr()
    a.eps_mode, a.math = eps_mode, math_mode
    a.eps_act = _ptr(eps_act) if eps_mode == L.EPS_MEMORY else None
    a.eps_b = _ptr(eps_b) if eps_mode == L.EPS_MEMORY else None
    a.seed, a.layer_id, a.sample_offset = seed & 0xFFFFFFFFFFFFFFFF, layer_id, sample_offset & 0xFFFFFFFF
    a.sample_counter = _ptr(sample_counter)
    a.sample_group, a.sample_group_stride = int(sample_group), int(sample_group_stride)
    a.form = int(form)
    a.eps_act_dump, a.eps_b_dump = _ptr(da), _ptr(db)
    a.sigma_p, a.want_kl, a.relu = float(sigma_p), int(want_kl), int(relu)
    a.workspace = _ptr(workspace) if want_kl else None
    a.workspace_bytes = workspace.numel() * 4 if (want_kl and workspace is not None) else 0
    a.kl_out = _ptr(kl3)
    a.y, a.y_dtype = y.data_ptr(), _dt(y)
    if x_sq is not None:
        if x_sq.dtype != torch.bfloat16 or tuple(x_sq.shape) != tuple(xs.shape) or not x_sq.is_contiguous():
            raise BnnHipError("x_sq must be a contiguous bfloat16 tensor shaped like x")
        a.x_sq = x_sq.data_ptr()
    if w_frag is not None:
        a.w_frag = w_frag.data_ptr()
    if out_sq is not None:
        if out_sq.dtype != torch.bfloat16 or out_sq.numel() != y.numel():
            raise BnnHipError("out_sq must be bfloat16 shaped like y")
        a.y_sq = out_sq.data_ptr()
    v = None
    if want_v:                                       # the variance the kernel sampled from: saved for bnn_lr_linear_bwd
        v = torch.empty(tuple(y.shape), dtype=torch.float32, device=y.device)
        a.v_out = v.data_ptr()
    hfac = None
    if want_hfac:                                    # eps_act / (2 sqrt(v)): lets bnn_lr_linear_bwd skip its preparation launch
        hfac = torch.empty(tuple(y.shape), dtype=torch.float32, device=y.device)
        a.hfac_out = hfac.data_ptr()
    y16 = None
    if want_y16:                                     # fp32 y for the backward, bf16 y for the next layer's forward
        if y.dtype != torch.float32:
            raise BnnHipError("want_y16 goes with fp32 y")
        y16 = torch.empty(tuple(y.shape), dtype=torch.bfloat16, device=y.device)
        a.y_bf16_copy = y16.data_ptr()
    if split_scratch is not None:
        a.split_scratch = split_scratch.data_ptr()
        a.split_scratch_bytes = split_scratch.numel() * split_scratch.element_size()
    y_lo = None
    if math_mode == L.MATH_BF16X3:
        if x_lo.dtype != torch.bfloat16 or tuple(x_lo.shape) != tuple(xs.shape) or not x_lo.is_contiguous():
            raise BnnHipError("x_lo must be a contiguous bfloat16 tensor shaped like x")
        require_device(x_lo)
        a.x_lo = x_lo.data_ptr()
        if y.dtype == torch.bfloat16:
            y_lo = out_lo if out_lo is not None else torch.empty(tuple(y.shape), dtype=torch.bfloat16, device=dev)
            if y_lo.dtype != torch.bfloat16 or y_lo.numel() != y.numel() or not y_lo.is_contiguous():
                raise BnnHipError("out_lo must be a contiguous bf16 tensor shaped like y")
            a.y_lo = y_lo.data_ptr()
    rd = None
    if rider is not None:
        rw = [_f32c(rider[k], k) for k in ("w_mu", "w_rho", "b_mu", "b_rho")]
        require_device(*rw, rider["w_frag"], rider["workspace"])
        rd = L.LrRider()
        rd.struct_bytes = C.sizeof(L.LrRider)
        rd.in_features, rd.out_features = int(rw[0].shape[0]), int(rw[0].shape[1])
        rd.w_mu, rd.w_rho, rd.b_mu, rd.b_rho = (t.data_ptr() for t in rw)
        rd.w_frag, rd.w_frag_bytes = rider["w_frag"].data_ptr(), rider["w_frag"].numel() * rider["w_frag"].element_size()
        rd.kl_workspace = rider["workspace"].data_ptr()
        rd.kl_workspace_bytes = rider["workspace"].numel() * rider["workspace"].element_size()
        a.rider = C.pointer(rd)
        rd = (rd, rw, rider["w_frag"], rider["workspace"])
    res = dict(y=y, y_sq=out_sq, workspace=workspace, kl3=kl3, eps_act=da, eps_b=db, v=v, y16=y16, hfac=hfac, y_lo=y_lo)
    keep = (xs, w_mu, w_rho, b_mu, b_rho, eps_act, eps_b, sample_counter, x_sq, w_frag, out_sq, workspace, split_scratch, rd, x_lo, y_lo)
    a._keep = keep                    # (the structure owns what its pointers refer to: engine.GraphedElbo(capture="calls") replays it)
    return a, res, keep


def lr_linear_fwd(x, w_mu, w_rho, b_mu, b_rho, **kw):
    """K3.  Weights are [in, out].  Returns dict(y, workspace, kl3, eps_act, eps_b)."""
    lib = L.load()
    a, res, keep = _lr_build(x, w_mu, w_rho, b_mu, b_rho, **kw)
    L.check(lib.bnn_lr_linear_fwd(C.byref(a), _stream()), "bnn_lr_linear_fwd")
    return res


def lr_final_fwd(layer_args: tuple, layer_kw: dict, fin_kw: dict):
    """Last LR layer + ELBO finalize through bnn_lr_final_fwd (one launch when the layer is narrow and the evaluation
    has few samples, else the two launches).  `fin_kw["workspaces"]` lists the KL workspaces of ALL layers (the last
    one's is filled only by the two-launch form); `logits` is taken from the layer call.
    Returns (layer result dict, finalize result dict)."""
    lib = L.load()
    a, res, keep1 = _lr_build(*layer_args, **layer_kw)
    fin_kw = dict(fin_kw)
    fin_kw["logits"] = res["y"]
    f, out, keep2 = _fin_build(**fin_kw)
    L.check(lib.bnn_lr_final_fwd(C.byref(a), C.byref(f), _stream()), "bnn_lr_final_fwd")
    return res, out


def lr_plan(x, w_mu, w_rho, b_mu, b_rho, **kw) -> dict:
    """bnn_lr_plan: the launch geometry lr_linear_fwd would use for these arguments (no launch)."""
    a, res, keep = _lr_build(x, w_mu, w_rho, b_mu, b_rho, **kw)
    pl = L.Plan()
    L.check(L.load().bnn_lr_plan(C.byref(a), C.byref(pl)), "bnn_lr_plan")
    return _plan_dict(pl)


def gauss_kl(mu: torch.Tensor, rho: torch.Tensor, sigma_p: float) -> torch.Tensor:
    """K2.  Returns float32[4] = (KL, sum log sigma, sum sigma^2, sum mu^2) on the device."""
    lib = L.load()
    require_device(mu, rho)
    mu, rho = _f32c(mu, "mu"), _f32c(rho, "rho")
    if mu.numel() != rho.numel():
        raise BnnHipError("mu and rho must have the same number of elements")
    n = mu.numel()
    ws = torch.empty(lib.bnn_gauss_kl_workspace_bytes(n) // 4, dtype=torch.float32, device=mu.device)
    out = torch.empty(4, dtype=torch.float32, device=mu.device)
    L.check(lib.bnn_gauss_kl(mu.data_ptr(), rho.data_ptr(), n, float(sigma_p), ws.data_ptr(), ws.numel() * 4,
                             out.data_ptr(), _stream()), "bnn_gauss_kl")
    return out


def _fin_build(*, workspaces, layer_in, layer_out, local_reparam: bool, prior: PriorSpec, n_samples: int,
               logits: Optional[torch.Tensor], target: Optional[torch.Tensor], mode: Optional[str],
               nll_sigma: float = 1.0, sample_counter=None, sample_counter_inc: int = 0, out=None, sums=None,
               ticket=None, scratch=None, group_samples: int = 0, loss=None):
    """`group_samples` g > 0: the n_samples are G = n_samples / g independent minibatches of g MC samples each;
    `target` may then hold one target block per minibatch ([G, batch] / [G, batch, classes]) and `sums` is [G, 4].
    `loss` = dict(beta=device scalar, total_samples=, grad_scale=): the training step's tail (bnn_loss_args); its
    results come back as out["loss"] = (out4, g_a, g_b, g_kl3, g_logits)."""
    n_layers = len(workspaces)
    dev = logits.device if logits is not None else workspaces[0].device
    a = L.FinalizeArgs()
    a.struct_bytes = C.sizeof(L.FinalizeArgs)
    a.n_layers, a.local_reparam, a.n_samples = n_layers, int(local_reparam), n_samples
    for i, (w, ki, ko) in enumerate(zip(workspaces, layer_in, layer_out)):
        require_device(w)
        a.layer_workspace[i] = w.data_ptr()
        a.layer_in[i], a.layer_out[i] = ki, ko
    a.prior = prior.c()
    out = {**dict(log_prior=None, log_q=None, kl=None, nll=None), **(out or {})}
    preset = {k for k, v in out.items() if v is not None}
    if n_layers:
        for key in (("kl",) if local_reparam else ("log_prior", "log_q")):
            if key not in preset:
                out[key] = torch.empty(n_samples, dtype=torch.float32, device=dev)
    keep = []
    if logits is not None:
        require_device(logits, target)
        lg = _f32c(logits, "logits")
        S, B, Cc = lg.shape
        if S != n_samples:
            raise BnnHipError("logits must be [samples,batch,classes]")
        G = n_samples // group_samples if group_samples else 1
        if group_samples and n_samples % group_samples:
            raise BnnHipError("group_samples must divide n_samples")
        if mode == "classification":
            tg = target.to(torch.int64).contiguous()
            if tg.numel() not in (B, G * B):
                raise BnnHipError("classification target must have `batch` elements (per minibatch)")
            a.nll_mode = L.NLL_CLASSIFICATION
            per_group = tg.numel() == G * B and G > 1
        elif mode == "regression":
            tg = _f32c(target.to(torch.float32), "target")
            if tg.numel() not in (B * Cc, G * B * Cc):
                raise BnnHipError("regression target must match the output shape (per minibatch)")
            a.nll_mode = L.NLL_REGRESSION
            per_group = tg.numel() == G * B * Cc and G > 1
        else:
            raise Exception("Training mode must be either 'regression' or 'classification'")
        a.target_per_group = int(per_group)
        keep += [lg, tg]
        a.batch, a.classes = B, Cc
        a.logits, a.target, a.nll_sigma = lg.data_ptr(), tg.data_ptr(), float(nll_sigma)
        if "nll" not in preset:
            out["nll"] = torch.empty(n_samples, dtype=torch.float32, device=dev)
    a.sample_counter, a.sample_counter_inc = _ptr(sample_counter), int(sample_counter_inc)
    a.sums = _ptr(sums)
    a.group_samples = int(group_samples)
    a.ticket = _ptr(ticket)
    a.scratch = _ptr(scratch)
    a.scratch_bytes = scratch.numel() * scratch.element_size() if scratch is not None else 0
    a.log_prior, a.log_q, a.kl, a.nll = _ptr(out["log_prior"]), _ptr(out["log_q"]), _ptr(out["kl"]), _ptr(out["nll"])
    keep += [sample_counter, sums, ticket, scratch] + list(workspaces)
    if loss is not None:
        if logits is None or group_samples:
            raise BnnHipError("the loss tail needs the logits of ONE evaluation")
        require_device(loss["beta"])
        la = L.LossArgs()
        res = (torch.empty(4, dtype=torch.float32, device=dev), torch.empty(n_samples, dtype=torch.float32, device=dev),
               torch.empty(n_samples, dtype=torch.float32, device=dev), torch.empty(3, dtype=torch.float32, device=dev),
               torch.empty_like(lg))
        la.beta, la.total_samples, la.grad_scale = loss["beta"].data_ptr(), float(loss["total_samples"]), float(loss.get("grad_scale", 1.0))
        la.out4, la.g_a, la.g_b, la.g_kl3, la.g_logits = (t.data_ptr() for t in res)
        a.loss = C.pointer(la)
        out["loss"] = res
        keep += [la, loss["beta"]] + list(res)
    a._keep = keep
    return a, out, keep


def elbo_finalize(**kw):
    """K4.  Returns dict(log_prior, log_q, kl, nll): float32[n_samples] tensors (or None)."""
    lib = L.load()
    a, out, keep = _fin_build(**kw)
    L.check(lib.bnn_elbo_finalize(C.byref(a), _stream()), "bnn_elbo_finalize")
    return out


def bbb_final_fwd(layer_args: tuple, layer_kw: dict, fin_kw: dict):
    """Last BBB layer + ELBO finalize through bnn_bbb_final_fwd (one launch when the layer is a
    single feature tile).  `fin_kw` must not carry `logits`/`workspaces` for the last layer:
    they are taken from the layer call.  Returns (layer result dict, finalize result dict)."""
    lib = L.load()
    a, res, keep1 = _bbb_build(*layer_args, **layer_kw)
    fin_kw = dict(fin_kw)
    if layer_kw.get("w_sampled") is None:              # (a pre-sampled layer: its statistics workspace, the sampler's, is
        fin_kw["workspaces"] = list(fin_kw["workspaces"]) + [res["workspace"]]     # already the last of fin_kw's)
    fin_kw["logits"] = res["y"]
    f, out, keep2 = _fin_build(**fin_kw)
    L.check(lib.bnn_bbb_final_fwd(C.byref(a), C.byref(f), _stream()), "bnn_bbb_final_fwd")
    return res, out


def philox_normal(seed: int, tensor_id: int, sample_offset: int, n_samples: int, rows: int, cols: int,
                  device) -> torch.Tensor:
    """The on-chip epsilon stream, materialised: float32[n_samples, rows, cols]."""
    lib = L.load()
    if torch.device(device).type != "cuda":
        raise BnnHipError("bnn_hip.philox_normal needs a ROCm device")
    eps = torch.empty((n_samples, rows, cols), dtype=torch.float32, device=device)
    L.check(lib.bnn_philox_normal(eps.data_ptr(), seed & 0xFFFFFFFFFFFFFFFF, tensor_id, sample_offset & 0xFFFFFFFF,
                                  n_samples, rows, cols, _stream()), "bnn_philox_normal")
    return eps


def cast_bf16(x: torch.Tensor, out: Optional[torch.Tensor] = None, out_sq: Optional[torch.Tensor] = None,
              want_sq: bool = False):
    """fp32 -> bf16 copy of a contiguous device tensor (one tiny kernel); with `want_sq` also
    x*x in bf16.  Returns out, or (out, out_sq)."""
    lib = L.load()
    require_device(x)
    x = _f32c(x, "x")
    if out is None:
        out = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    if want_sq and out_sq is None:
        out_sq = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    L.check(lib.bnn_cast_bf16(x.data_ptr(), out.data_ptr(), _ptr(out_sq), x.numel(), _stream()), "bnn_cast_bf16")
    return (out, out_sq) if (want_sq or out_sq is not None) else out


def lr_prepare(w_mu, w_rho, b_mu, b_rho, workspace=None, out=None, x3: bool = False):
    """bnn_lr_prepare: bf16 (M, sigma^2) in MFMA fragment order + the KL sums into `workspace` (`x3`: bnn_lr_prepare_x3 --
    the fragments of the split-bf16 math mode, with the low part of M as a third plane).  Returns (w_frag, workspace)."""
    lib = L.load()
    require_device(w_mu, w_rho, b_mu, b_rho)
    w_mu, w_rho = _f32c(w_mu, "weight_mu"), _f32c(w_rho, "weight_rho")
    b_mu, b_rho = _f32c(b_mu, "bias_mu"), _f32c(b_rho, "bias_rho")
    K, N = w_mu.shape
    nbytes = (lib.bnn_lr_prepare_x3_bytes if x3 else lib.bnn_lr_prepare_bytes)(K, N)
    if out is None:
        out = torch.empty(nbytes // 4, dtype=torch.float32, device=w_mu.device)
    if workspace is None:
        workspace = lr_workspace(N, w_mu.device)
    fn = lib.bnn_lr_prepare_x3 if x3 else lib.bnn_lr_prepare
    L.check(fn(w_mu.data_ptr(), w_rho.data_ptr(), b_mu.data_ptr(), b_rho.data_ptr(), K, N,
               out.data_ptr(), out.numel() * 4, workspace.data_ptr(), workspace.numel() * 4, _stream()),
            "bnn_lr_prepare")
    return out, workspace


def lr_prepare_many(jobs: Sequence[dict], x3: bool = False):
    """bnn_lr_prepare_many: the prepared operands of several layers in ONE launch.  Each job: dict(w_mu, w_rho, b_mu, b_rho,
    workspace, out) with `out` / `workspace` as in lr_prepare (allocated when absent).  Returns [(w_frag, workspace), ...]."""
    lib = L.load()
    if not 1 <= len(jobs) <= L.PREPARE_MANY_MAX:
        raise BnnHipError(f"lr_prepare_many: 1 .. {L.PREPARE_MANY_MAX} layers per launch")
    arr = (L.LrPrepareJob * len(jobs))()
    keep, res = [], []
    for j, q in enumerate(jobs):
        require_device(q["w_mu"], q["w_rho"], q["b_mu"], q["b_rho"])
        w_mu, w_rho = _f32c(q["w_mu"], "weight_mu"), _f32c(q["w_rho"], "weight_rho")
        b_mu, b_rho = _f32c(q["b_mu"], "bias_mu"), _f32c(q["b_rho"], "bias_rho")
        K, N = w_mu.shape
        nbytes = (lib.bnn_lr_prepare_x3_bytes if x3 else lib.bnn_lr_prepare_bytes)(K, N)
        out = q.get("out")
        if out is None:
            out = torch.empty(nbytes // 4, dtype=torch.float32, device=w_mu.device)
        ws = q.get("workspace")
        if ws is None:
            ws = lr_workspace(N, w_mu.device)
        keep += [w_mu, w_rho, b_mu, b_rho, out, ws]
        a = arr[j]
        a.w_mu, a.w_rho, a.b_mu, a.b_rho = w_mu.data_ptr(), w_rho.data_ptr(), b_mu.data_ptr(), b_rho.data_ptr()
        a.in_features, a.out_features = K, N
        a.w_frag, a.w_frag_bytes = out.data_ptr(), out.numel() * 4
        a.kl_workspace, a.kl_workspace_bytes = ws.data_ptr(), ws.numel() * 4
        res.append((out, ws))
    L.check(lib.bnn_lr_prepare_many(arr, len(jobs), int(bool(x3)), _stream()), "bnn_lr_prepare_many")
    return res


def _grad_outputs(out, w_mu, w_rho, b_mu, b_rho):
    """Gradient destinations: fresh tensors, or the caller's (e.g. views of one flat all-reduce bucket)."""
    if out is None:
        return torch.empty_like(w_mu), torch.empty_like(w_rho), torch.empty_like(b_mu), torch.empty_like(b_rho)
    for o, p_ in zip(out, (w_mu, w_rho, b_mu, b_rho)):
        if o.dtype != torch.float32 or tuple(o.shape) != tuple(p_.shape) or not o.is_contiguous() or o.device != p_.device:
            raise BnnHipError("gradient outputs must be contiguous float32 tensors shaped like their parameters")
    return tuple(out)


def bbb_linear_bwd(x, gy, y, w_mu, w_rho, b_mu, b_rho, *, n_samples: int, prior: PriorSpec, math_mode: int, relu: bool,
                   eps_mode: int, eps_w=None, eps_b=None, seed: int = 0, layer_id: int = 0, sample_offset: int = 0,
                   g_log_prior=None, g_log_q=None, want_gx: bool = True, sample_counter=None, out=None,
                   gx_relu_mask: bool = False, w_sampled=None, w_sampled_t=None, gy16=None, want_gx16: bool = False):
    """F1: backward of K1 (bnn_bbb_linear_bwd).  All tensors fp32.  Returns
    (g_w_mu, g_w_rho, g_b_mu, g_b_rho, g_x[S,B,K] | None), with `want_gx16` also g_x in bf16 as a sixth element.
    `w_sampled_t` (bf16 [S,in,out], the forward's wt_out) / `gy16` (bf16 copy of gy): the input gradient as the
    forward's matmul-only launch."""
    lib = L.load()
    require_device(x, gy, y, w_mu, w_rho, b_mu, b_rho, eps_w, eps_b, g_log_prior, g_log_q)
    w_mu, w_rho = _f32c(w_mu, "weight_mu"), _f32c(w_rho, "weight_rho")
    b_mu, b_rho = _f32c(b_mu, "bias_mu"), _f32c(b_rho, "bias_rho")
    N, K = w_mu.shape
    xs, B, Kx, per_sample = _x3(_f32c(x, "x"), n_samples)
    gy = _f32c(gy, "gy")
    if Kx != K or gy.numel() != n_samples * B * N:
        raise BnnHipError("bbb_linear_bwd: shape mismatch")
    dev = xs.device
    a = L.BbbBwdArgs()
    a.struct_bytes = C.sizeof(L.BbbBwdArgs)
    a.n_samples, a.batch, a.in_features, a.out_features = n_samples, B, K, N
    a.x, a.x_per_sample, a.relu = xs.data_ptr(), per_sample, int(relu)
    a.gy = gy.data_ptr()
    if relu:
        y = _f32c(y, "y")
        a.y = y.data_ptr()
    a.w_mu, a.w_rho, a.b_mu, a.b_rho = w_mu.data_ptr(), w_rho.data_ptr(), b_mu.data_ptr(), b_rho.data_ptr()
    a.eps_mode, a.math = eps_mode, _exact_unless_bf16(math_mode)
    if eps_mode == L.EPS_MEMORY:
        eps_w, eps_b = _f32c(eps_w, "eps_w"), _f32c(eps_b, "eps_b")
        a.eps_w, a.eps_b = eps_w.data_ptr(), eps_b.data_ptr()
    a.seed, a.layer_id, a.sample_offset = seed & 0xFFFFFFFFFFFFFFFF, layer_id, sample_offset & 0xFFFFFFFF
    a.prior = prior.c()
    glp = _f32c(g_log_prior, "g_log_prior") if g_log_prior is not None else None
    glq = _f32c(g_log_q, "g_log_q") if g_log_q is not None else None
    a.g_log_prior, a.g_log_q = _ptr(glp), _ptr(glq)
    g_wmu, g_wrho, g_bmu, g_brho = _grad_outputs(out, w_mu, w_rho, b_mu, b_rho)
    gx = torch.empty((n_samples, B, K), dtype=torch.float32, device=dev) if want_gx else None
    a.g_w_mu, a.g_w_rho, a.g_b_mu, a.g_b_rho = g_wmu.data_ptr(), g_wrho.data_ptr(), g_bmu.data_ptr(), g_brho.data_ptr()
    a.g_x = _ptr(gx)
    a.gx_relu_mask = int(bool(gx_relu_mask) and want_gx)
    if w_sampled is not None and want_gx:
        require_device(w_sampled)
        if w_sampled.dtype != torch.bfloat16 or not w_sampled.is_contiguous() or w_sampled.numel() != n_samples * N * K:
            raise BnnHipError("bbb_linear_bwd: w_sampled must be contiguous bf16 [samples,out,in]")
        a.w_sampled = w_sampled.data_ptr()
    if w_sampled_t is not None and want_gx:
        require_device(w_sampled_t, gy16)
        if w_sampled_t.dtype != torch.bfloat16 or not w_sampled_t.is_contiguous() or tuple(w_sampled_t.shape) != (n_samples, K, N):
            raise BnnHipError("bbb_linear_bwd: w_sampled_t must be contiguous bf16 [samples,in,out]")
        a.w_sampled_t = w_sampled_t.data_ptr()
        if gy16 is not None:
            if gy16.dtype != torch.bfloat16 or not gy16.is_contiguous() or gy16.numel() != gy.numel():
                raise BnnHipError("bbb_linear_bwd: gy16 must be a contiguous bf16 copy of gy")
            a.gy_bf16 = gy16.data_ptr()
    gx16 = None
    if want_gx16 and want_gx:
        gx16 = torch.empty((n_samples, B, K), dtype=torch.bfloat16, device=dev)
        a.g_x_bf16 = gx16.data_ptr()
    ws = torch.empty(lib.bnn_bbb_linear_bwd_workspace_bytes(n_samples, B, N) // 4, dtype=torch.float32, device=dev)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    a.sample_counter = _ptr(sample_counter)
    L.check(lib.bnn_bbb_linear_bwd(C.byref(a), _stream()), "bnn_bbb_linear_bwd")
    if want_gx16:
        return g_wmu, g_wrho, g_bmu, g_brho, gx, gx16
    return g_wmu, g_wrho, g_bmu, g_brho, gx


def lr_linear_bwd(x, gy, y, v, w_mu, w_rho, b_mu, b_rho, *, n_samples: int, sigma_p: float, relu: bool, eps_mode: int,
                  eps_act=None, eps_b=None, seed: int = 0, layer_id: int = 0, sample_offset: int = 0, g_kl=None,
                  want_gx: bool = True, sample_counter=None, out=None, gx_relu_mask: bool = False, math_mode: int = L.MATH_F32,
                  hfac=None):
    """F1: backward of K3 (bnn_lr_linear_bwd).  All tensors fp32; `v` is the variance the forward
    saved (lr_linear_fwd(want_v=True)), or None with `hfac` (lr_linear_fwd(want_hfac=True); relu must be False: no
    preparation launch then); g_kl float[3] = upstream grads of (kl, weight_kl, bias_kl).
    Returns (g_w_mu, g_w_rho, g_b_mu, g_b_rho, g_x[S,B,K] | None)."""
    lib = L.load()
    require_device(x, gy, y, v, hfac, w_mu, w_rho, b_mu, b_rho, eps_act, eps_b, g_kl)
    w_mu, w_rho = _f32c(w_mu, "weight_mu"), _f32c(w_rho, "weight_rho")
    b_mu, b_rho = _f32c(b_mu, "bias_mu"), _f32c(b_rho, "bias_rho")
    K, N = w_mu.shape
    xs, B, Kx, per_sample = _x3(_f32c(x, "x"), n_samples)
    gy = _f32c(gy, "gy")
    v = _f32c(v, "v") if v is not None else None
    hfac = _f32c(hfac, "hfac") if hfac is not None else None
    if v is None and (hfac is None or relu):
        raise BnnHipError("lr_linear_bwd: needs the forward's v (or its hfac for a layer without a fused ReLU)")
    if Kx != K or gy.numel() != n_samples * B * N or any(t_ is not None and t_.numel() != gy.numel() for t_ in (v, hfac)):
        raise BnnHipError("lr_linear_bwd: shape mismatch")
    dev = xs.device
    a = L.LrBwdArgs()
    a.struct_bytes = C.sizeof(L.LrBwdArgs)
    a.n_samples, a.batch, a.in_features, a.out_features = n_samples, B, K, N
    a.x, a.x_per_sample, a.relu = xs.data_ptr(), per_sample, int(relu)
    a.gy, a.v, a.hfac = gy.data_ptr(), _ptr(v), _ptr(hfac)
    if relu:
        y = _f32c(y, "y")
        a.y = y.data_ptr()
    a.w_mu, a.w_rho, a.b_mu, a.b_rho = w_mu.data_ptr(), w_rho.data_ptr(), b_mu.data_ptr(), b_rho.data_ptr()
    a.eps_mode, a.math = eps_mode, _exact_unless_bf16(int(math_mode))
    if eps_mode == L.EPS_MEMORY:
        eps_act, eps_b = _f32c(eps_act, "eps_act"), _f32c(eps_b, "eps_b")
        a.eps_act, a.eps_b = eps_act.data_ptr(), eps_b.data_ptr()
    a.seed, a.layer_id, a.sample_offset = seed & 0xFFFFFFFFFFFFFFFF, layer_id, sample_offset & 0xFFFFFFFF
    a.sigma_p = float(sigma_p)
    gk = _f32c(g_kl, "g_kl") if g_kl is not None else None
    a.g_kl = _ptr(gk)
    g_wmu, g_wrho, g_bmu, g_brho = _grad_outputs(out, w_mu, w_rho, b_mu, b_rho)
    gx = torch.empty((n_samples, B, K), dtype=torch.float32, device=dev) if want_gx else None
    a.g_w_mu, a.g_w_rho, a.g_b_mu, a.g_b_rho = g_wmu.data_ptr(), g_wrho.data_ptr(), g_bmu.data_ptr(), g_brho.data_ptr()
    a.g_x = _ptr(gx)
    a.gx_relu_mask = int(bool(gx_relu_mask) and want_gx)
    ws = torch.empty(lib.bnn_lr_linear_bwd_workspace_bytes(n_samples, B, K, N, int(want_gx)) // 4, dtype=torch.float32,
                     device=dev)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    a.sample_counter = _ptr(sample_counter)
    L.check(lib.bnn_lr_linear_bwd(C.byref(a), _stream()), "bnn_lr_linear_bwd")
    return g_wmu, g_wrho, g_bmu, g_brho, gx


def mc_softmax_mean(logits: torch.Tensor, scale: float, want_preds: bool = True, out_probs: Optional[torch.Tensor] = None,
                    out_preds: Optional[torch.Tensor] = None):
    """F3: probs[B,C] = scale * sum_s softmax(logits[s]), preds[B] = argmax (bnn_mc_softmax_mean).  `out_probs` / `out_preds`:
    static buffers of a captured evaluation."""
    lib = L.load()
    require_device(logits, out_probs, out_preds)
    lg = _f32c(logits, "logits")
    S, B, Cc = lg.shape
    if out_probs is not None and (out_probs.dtype != torch.float32 or tuple(out_probs.shape) != (B, Cc) or not out_probs.is_contiguous()):
        raise BnnHipError("mc_softmax_mean: out_probs must be a contiguous float32 [batch, classes] tensor")
    if out_preds is not None and (out_preds.dtype != torch.int64 or tuple(out_preds.shape) != (B,) or not out_preds.is_contiguous()):
        raise BnnHipError("mc_softmax_mean: out_preds must be a contiguous int64 [batch] tensor")
    probs = out_probs if out_probs is not None else torch.empty((B, Cc), dtype=torch.float32, device=lg.device)
    preds = out_preds if out_preds is not None else (torch.empty(B, dtype=torch.int64, device=lg.device) if want_preds else None)
    L.check(lib.bnn_mc_softmax_mean(lg.data_ptr(), S, B, Cc, float(scale), probs.data_ptr(), _ptr(preds), _stream()),
            "bnn_mc_softmax_mean")
    return probs, preds


class Predictive(NamedTuple):
    """Predictive summaries of MC outputs (bnn_mc_predictive).  Classification fills probs / preds / the three entropies,
    regression mean / variance / predictive_variance / quantiles; the other mode's fields are None (quantiles too when no
    level was asked for).  Shapes [B, ...] for one minibatch, [G, B, ...] for G stacked ones; quantiles [Q, (G,) B, out]."""
    probs: Optional[torch.Tensor] = None
    preds: Optional[torch.Tensor] = None
    predictive_entropy: Optional[torch.Tensor] = None
    expected_entropy: Optional[torch.Tensor] = None
    mutual_information: Optional[torch.Tensor] = None
    mean: Optional[torch.Tensor] = None
    variance: Optional[torch.Tensor] = None
    predictive_variance: Optional[torch.Tensor] = None
    quantiles: Optional[torch.Tensor] = None


def quantile_levels(quantiles) -> tuple:
    """The quantile levels as floats, checked as bnn_mc_predictive checks them (ahead of any allocation)."""
    q = tuple(float(v) for v in (quantiles or ()))
    if len(q) > L.PREDICTIVE_MAX_QUANTILES:
        raise BnnHipError(f"at most {L.PREDICTIVE_MAX_QUANTILES} quantile levels")
    if not all(0.0 <= v <= 1.0 for v in q):             # (NaN fails)
        raise BnnHipError(f"quantile levels must lie in [0, 1], got {q}")
    return q


def predictive_buffers(mode: str, G: int, B: int, Cc: int, device, quantiles=(), partial: bool = False) -> Predictive:
    """Output tensors of bnn_mc_predictive for logits [G, S, B, Cc].  `partial`: a rank's share of a sample-sharded job --
    the buffers for the optional outputs too (they receive the combined values: engine.combine_predictive)."""
    f = dict(dtype=torch.float32, device=device)
    if mode == "classification":
        return Predictive(probs=torch.empty((G, B, Cc), **f), preds=torch.empty((G, B), dtype=torch.int64, device=device),
                          predictive_entropy=torch.empty((G, B), **f), expected_entropy=torch.empty((G, B), **f),
                          mutual_information=torch.empty((G, B), **f))
    if mode == "regression":
        q = quantile_levels(quantiles)
        return Predictive(mean=torch.empty((G, B, Cc), **f), variance=torch.empty((G, B, Cc), **f),
                          predictive_variance=torch.empty((G, B, Cc), **f),
                          quantiles=torch.empty((len(q), G, B, Cc), **f) if q else None)
    raise Exception("Training mode must be either 'regression' or 'classification'")


def mc_predictive(logits: torch.Tensor, mode: str, *, groups: int = 1, scale: Optional[float] = None, sigma: float = 1.0,
                  quantiles=(), partial: bool = False, out: Optional[Predictive] = None) -> Predictive:
    """F3: bnn_mc_predictive over logits [groups * S, B, C] (g-major, the layout of a stacked evaluation's output).
    Returns a Predictive of [groups, B, ...] tensors (`out`: static buffers of a captured evaluation, from
    predictive_buffers).  `scale`: classification's weight of the sums, 1 / S by default.  `partial`: only what a rank of
    a sample-sharded job contributes -- classification probs and expected_entropy (pass scale = 1 / global samples),
    regression mean and variance of the local samples; the other fields are left for engine.combine_predictive."""
    lib = L.load()
    require_device(logits)
    lg = _f32c(logits, "logits")
    if lg.dim() != 3 or lg.shape[0] % groups:
        raise BnnHipError("mc_predictive: logits must be [groups * samples, batch, outputs]")
    G = int(groups)
    S, B, Cc = lg.shape[0] // G, lg.shape[1], lg.shape[2]
    q = quantile_levels(quantiles) if mode == "regression" else ()
    if partial and q:
        raise BnnHipError("mc_predictive: quantiles of sample-sharded outputs are not supported")
    if out is None:
        out = predictive_buffers(mode, G, B, Cc, lg.device, q)
    want = dict(probs=(G, B, Cc), preds=(G, B), predictive_entropy=(G, B), expected_entropy=(G, B), mutual_information=(G, B),
                mean=(G, B, Cc), variance=(G, B, Cc), predictive_variance=(G, B, Cc), quantiles=(len(q), G, B, Cc))
    for name, tns in zip(out._fields, out):
        if tns is None:
            continue
        require_device(tns)
        dt = torch.int64 if name == "preds" else torch.float32
        if tuple(tns.shape) != want[name] or tns.dtype != dt or not tns.is_contiguous():
            raise BnnHipError(f"mc_predictive: out.{name} must be a contiguous {dt} tensor of shape {want[name]}")
    a = L.McPredictiveArgs()
    a.struct_bytes = C.sizeof(L.McPredictiveArgs)
    a.groups, a.n_samples, a.batch, a.classes = G, S, B, Cc
    a.logits = lg.data_ptr()
    if mode == "classification":
        a.mode = L.NLL_CLASSIFICATION
        a.scale = float(1.0 / S if scale is None else scale)
        a.probs, a.expected_entropy = out.probs.data_ptr(), out.expected_entropy.data_ptr()
        if not partial:
            a.preds, a.predictive_entropy, a.mutual_information = (_ptr(out.preds), _ptr(out.predictive_entropy),
                                                                   _ptr(out.mutual_information))
    elif mode == "regression":
        a.mode = L.NLL_REGRESSION
        a.sigma = float(sigma)
        a.mean, a.variance = out.mean.data_ptr(), out.variance.data_ptr()
        if not partial:
            a.predictive_variance = _ptr(out.predictive_variance)
        a.n_quantiles = len(q)
        for i, v in enumerate(q):
            a.quantile[i] = v
        if q:
            if out.quantiles is None:
                raise BnnHipError("mc_predictive: quantile levels need out.quantiles")
            a.quantiles = out.quantiles.data_ptr()
    else:
        raise Exception("Training mode must be either 'regression' or 'classification'")
    a._keep = (lg, out)               # (the structure owns what its pointers refer to: engine.GraphedElbo(capture="calls") replays it)
    L.check(lib.bnn_mc_predictive(C.byref(a), _stream()), "bnn_mc_predictive")
    return out


def elbo_loss(a, b, nll, beta, total_samples: int, local_reparam: bool, grad_scale: float = 1.0):
    """bnn_elbo_loss: returns (out4 {loss, mean a, mean b, mean nll}, g_a, g_b, g_nll, g_kl3)."""
    lib = L.load()
    require_device(a, b, nll, beta)
    S = nll.numel()
    dev = nll.device
    out4 = torch.empty(4, dtype=torch.float32, device=dev)
    g_a = torch.empty(S, dtype=torch.float32, device=dev)
    g_b = torch.empty(S, dtype=torch.float32, device=dev)
    g_nll = torch.empty(S, dtype=torch.float32, device=dev)
    g_kl3 = torch.empty(3, dtype=torch.float32, device=dev)
    L.check(lib.bnn_elbo_loss(a.data_ptr(), _ptr(b), nll.data_ptr(), beta.data_ptr(), S, float(total_samples),
                              float(grad_scale), int(local_reparam), out4.data_ptr(), g_a.data_ptr(), g_b.data_ptr(), g_nll.data_ptr(),
                              g_kl3.data_ptr(), _stream()), "bnn_elbo_loss")
    return out4, g_a, g_b, g_nll, g_kl3


def _nll_target(target, mode: str, B: int, Cc: int):
    if mode == "classification":
        tg, m = target.to(torch.int64).contiguous(), L.NLL_CLASSIFICATION
        if tg.numel() != B:
            raise BnnHipError("classification target must have `batch` elements")
    elif mode == "regression":
        tg, m = _f32c(target.to(torch.float32), "target"), L.NLL_REGRESSION
        if tg.numel() != B * Cc:
            raise BnnHipError("regression target must match the output shape")
    else:
        raise Exception("Training mode must be either 'regression' or 'classification'")
    return tg, m


def elbo_loss_nll_bwd(a, b, nll, beta, total_samples: int, local_reparam: bool, logits, target, mode: str,
                      sigma: float = 1.0, grad_scale: float = 1.0, out=None):
    """bnn_elbo_loss_nll_bwd: elbo_loss + nll_bwd in one launch.  Returns (out4, g_a, g_b, g_kl3, g_logits): fresh tensors, or
    `out` -- the caller's own five float32 buffers of those shapes (a captured step that keeps static outputs)."""
    lib = L.load()
    require_device(a, b, nll, beta, logits, target)
    lg = _f32c(logits, "logits")
    S, B, Cc = lg.shape
    if nll.numel() != S:
        raise BnnHipError("nll must have one element per MC sample")
    tg, m = _nll_target(target, mode, B, Cc)
    dev = nll.device
    if out is not None:
        out4, g_a, g_b, g_kl3, g_logits = out
        require_device(*out)
        for t_, n_ in zip(out, (4, S, S, 3, lg.numel())):
            if t_.dtype != torch.float32 or not t_.is_contiguous() or t_.numel() != n_:
                raise BnnHipError("elbo_loss_nll_bwd: out = (out4 [4], g_a [S], g_b [S], g_kl3 [3], g_logits like logits), contiguous float32")
    else:
        out4 = torch.empty(4, dtype=torch.float32, device=dev)
        g_a = torch.empty(S, dtype=torch.float32, device=dev)
        g_b = torch.empty(S, dtype=torch.float32, device=dev)
        g_kl3 = torch.empty(3, dtype=torch.float32, device=dev)
        g_logits = torch.empty_like(lg)
    L.check(lib.bnn_elbo_loss_nll_bwd(a.data_ptr(), _ptr(b), nll.data_ptr(), beta.data_ptr(), S, float(total_samples),
                                      float(grad_scale), int(local_reparam), out4.data_ptr(), g_a.data_ptr(), g_b.data_ptr(),
                                      g_kl3.data_ptr(), lg.data_ptr(), tg.data_ptr(), g_logits.data_ptr(), B, Cc, m,
                                      float(sigma), _stream()), "bnn_elbo_loss_nll_bwd")
    return out4, g_a, g_b, g_kl3, g_logits


def stage_inputs(src0, dst0, src1=None, dst1=None, word=None, value: float = 0.0, cast0=None):
    """bnn_stage_inputs: dst0 <- src0, dst1 <- src1 (same dtype, shape; contiguous device tensors), *word = value,
    one launch.  `cast0` (bf16, src0's shape, src0 fp32): also the bf16 copy of src0 (bnn_stage_inputs_cast)."""
    lib = L.load()
    require_device(src0, dst0, src1, dst1, word)
    for s_, d_ in ((src0, dst0), (src1, dst1)):
        if s_ is None:
            continue
        if s_.dtype != d_.dtype or s_.numel() != d_.numel() or not s_.is_contiguous() or not d_.is_contiguous():
            raise BnnHipError("stage_inputs: source and destination must be contiguous, same dtype and size")
    nb = lambda t: 0 if t is None else t.numel() * t.element_size()
    if cast0 is not None:
        require_device(cast0)
        if src0.dtype != torch.float32 or cast0.dtype != torch.bfloat16 or cast0.numel() != src0.numel() or not cast0.is_contiguous():
            raise BnnHipError("stage_inputs: cast0 must be a contiguous bf16 tensor of the fp32 src0's size")
        L.check(lib.bnn_stage_inputs_cast(_ptr(src0), _ptr(dst0), nb(src0), _ptr(src1), _ptr(dst1), nb(src1), _ptr(word),
                                          float(value), cast0.data_ptr(), _stream()), "bnn_stage_inputs_cast")
        return
    L.check(lib.bnn_stage_inputs(_ptr(src0), _ptr(dst0), nb(src0), _ptr(src1), _ptr(dst1), nb(src1), _ptr(word), float(value),
                                 _stream()), "bnn_stage_inputs")


def nll_bwd(logits, target, g_nll, mode: str, sigma: float = 1.0):
    """Gradient of the per-sample summed NLL w.r.t. logits[S,B,C] scaled by g_nll[S] (bnn_nll_bwd)."""
    lib = L.load()
    require_device(logits, target, g_nll)
    lg = _f32c(logits, "logits")
    S, B, Cc = lg.shape
    gn = _f32c(g_nll.reshape(-1), "g_nll")
    if gn.numel() != S:
        raise BnnHipError("g_nll must have one element per MC sample")
    tg, m = _nll_target(target, mode, B, Cc)
    out = torch.empty_like(lg)
    L.check(lib.bnn_nll_bwd(lg.data_ptr(), tg.data_ptr(), gn.data_ptr(), out.data_ptr(), S, B, Cc, m, float(sigma), _stream()),
            "bnn_nll_bwd")
    return out


def adam_step(params, grads, exp_avgs, exp_avg_sqs, *, lr: float, betas, eps: float, weight_decay: float, step: int = 0,
              lr_device=None, step_device=None, ticket=None, bump_counter=None, bump_by: int = 0):
    """F2: bnn_adam_step over lists of fp32 tensors (any number; 16 per launch; the gradients fp32 or bf16).  With `ticket` (zeroed device array
    of 16 uint32) the device step advances inside the first launch, which also adds bump_by to *bump_counter."""
    lib = L.load()
    n = len(params)
    for lo in range(0, n, L.ADAM_MAX_TENSORS):
        hi = min(n, lo + L.ADAM_MAX_TENSORS)
        a = L.AdamArgs()
        a.struct_bytes = C.sizeof(L.AdamArgs)
        a.n_tensors = hi - lo
        for j in range(lo, hi):
            p, g, m, v = params[j], grads[j], exp_avgs[j], exp_avg_sqs[j]
            require_device(p, g, m, v)
            for t_ in (p, m, v):
                if t_.dtype != torch.float32 or not t_.is_contiguous() or t_.numel() != p.numel():
                    raise BnnHipError("adam_step: tensors must be contiguous float32 of the parameter's size")
            if g.dtype not in (torch.float32, torch.bfloat16) or g.dtype != grads[lo].dtype or not g.is_contiguous() or \
                    g.numel() != p.numel():
                raise BnnHipError("adam_step: gradients must be contiguous float32 or bfloat16 (one dtype per launch) of the "
                                  "parameter's size")
            a.param[j - lo], a.grad[j - lo] = p.data_ptr(), g.data_ptr()
            a.exp_avg[j - lo], a.exp_avg_sq[j - lo] = m.data_ptr(), v.data_ptr()
            a.numel[j - lo] = p.numel()
        a.lr, a.beta1, a.beta2, a.eps, a.weight_decay = float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay)
        a.step = int(step)
        a.grad_dtype = _dt(grads[lo])
        a.lr_device = _ptr(lr_device)
        a.step_device = _ptr(step_device)
        a.step_advance = int(lo == 0)                   # the first launch of the step advances the device counter
        if lo == 0 and ticket is not None and step_device is not None:
            if ticket.numel() < 16 or ticket.element_size() != 4:
                raise BnnHipError("adam_step: ticket must be a zeroed array of 16 32-bit words")
            a.ticket = ticket.data_ptr()
            if bump_counter is not None:
                a.bump_counter, a.bump_by = bump_counter.data_ptr(), int(bump_by)
        elif bump_counter is not None and lo == 0:
            raise BnnHipError("adam_step: bump_counter needs a device step and a ticket word")
        L.check(lib.bnn_adam_step(C.byref(a), _stream()), "bnn_adam_step")


def softplus(rho: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sigma = log1p(exp(rho)) by bnn_softplus (one elementwise kernel)."""
    lib = L.load()
    require_device(rho)
    rho = _f32c(rho, "rho")
    if out is None:
        out = torch.empty_like(rho)
    L.check(lib.bnn_softplus(rho.data_ptr(), out.data_ptr(), rho.numel(), _stream()), "bnn_softplus")
    return out


def eval_prepare(rhos=(), sigmas=None, cast: Optional[torch.Tensor] = None, cast_out: Optional[torch.Tensor] = None,
                 cast_out_sq: Optional[torch.Tensor] = None, want_sq: bool = False, cast_out_lo: Optional[torch.Tensor] = None,
                 mus=None, pieces=None):
    """bnn_eval_prepare: sigma = softplus(rho) for every tensor of `rhos` and (optionally) the bf16 cast of `cast`
    (+ its squares; + `cast_out_lo`, the low plane bf16(x - bf16(x)) of the split-bf16 math mode) in ONE launch --
    everything of an evaluation that depends on no activation.  `cast_out` may be a piece-order buffer (pieces_activation).
    `mus` / `pieces` (lists beside `rhos`, entries may be None): the 2-D tensor's (mu, sigma) once more in piece order
    (param_pieces), by the same launch.
    Returns (list of sigma tensors, cast_out, cast_out_sq)."""
    lib = L.load()
    rhos = [_f32c(r, "rho") for r in rhos]
    require_device(*rhos, cast)
    if len(rhos) > L.PREPARE_MAX:
        raise BnnHipError(f"eval_prepare: at most {L.PREPARE_MAX} tensors per launch")
    if sigmas is None:
        sigmas = [torch.empty_like(r) for r in rhos]
    a = L.PrepareArgs()
    a.struct_bytes = C.sizeof(L.PrepareArgs)
    a.n_softplus = len(rhos)
    for i, (r, sg) in enumerate(zip(rhos, sigmas)):
        if sg.shape != r.shape or sg.dtype != torch.float32 or not sg.is_contiguous():
            raise BnnHipError("eval_prepare: sigma must be a contiguous fp32 tensor of rho's shape")
        a.rho[i], a.sigma[i], a.n[i] = r.data_ptr(), sg.data_ptr(), r.numel()
        pc = pieces[i] if pieces is not None else None
        if pc is not None:
            mu = _f32c(mus[i], "mu")
            require_device(mu, pc)
            if r.dim() != 2 or mu.shape != r.shape or pc.dtype != torch.float32 or not pc.is_contiguous() or \
                    pc.numel() != ((r.shape[0] + 15) // 16) * ((r.shape[1] + 31) // 32) * 1024:
                raise BnnHipError("eval_prepare: pieces[i] must be ops.param_pieces(out, in) of the [out, in] tensors mus[i] / rhos[i]")
            a.mu[i], a.pieces[i], a.rows[i], a.cols[i] = mu.data_ptr(), pc.data_ptr(), r.shape[0], r.shape[1]
            a._keep_mu = getattr(a, "_keep_mu", ()) + (mu,)
    if cast is not None:
        cast = _f32c(cast, "x")
        if cast_out is None:
            cast_out = torch.empty(cast.shape, dtype=torch.bfloat16, device=cast.device)
        if want_sq and cast_out_sq is None:
            cast_out_sq = torch.empty(cast.shape, dtype=torch.bfloat16, device=cast.device)
        a.cast_src, a.cast_dst, a.cast_dst_sq, a.cast_n = cast.data_ptr(), cast_out.data_ptr(), _ptr(cast_out_sq), cast.numel()
        ps = pieces_shape(cast_out)
        if ps is not None:                  # the cast in piece order (ops.pieces_activation of the input's shape)
            if tuple(ps) != tuple(cast.shape):
                raise BnnHipError(f"eval_prepare: cast_out is a piece-order buffer for {tuple(ps)}, the input is {tuple(cast.shape)}")
            a.cast_layout, a.cast_batch, a.cast_features = L.LAYOUT_PIECES, ps[-2], ps[-1]
        if cast_out_lo is not None:
            if cast_out_lo.dtype != torch.bfloat16 or cast_out_lo.numel() != cast.numel() or not cast_out_lo.is_contiguous():
                raise BnnHipError("eval_prepare: cast_out_lo must be a contiguous bf16 tensor of the input's size")
            require_device(cast_out_lo)
            a.cast_dst_lo = cast_out_lo.data_ptr()
    if not rhos and cast is None:
        return [], None, None
    L.check(lib.bnn_eval_prepare(C.byref(a), _stream()), "bnn_eval_prepare")
    return list(sigmas), cast_out, cast_out_sq


def ece_bins(probs: torch.Tensor, labels: torch.Tensor, bin_edges) -> torch.Tensor:
    """F3: bnn_ece.  probs fp32 [n, classes], labels int64[n] on the device, bin_edges a host float64 sequence.
    Returns float32 [1 + 3 * nbins] = (ece, then per bin count, corrects, confidence sum)."""
    lib = L.load()
    require_device(probs, labels)
    pr = _f32c(probs, "probs")
    if pr.dim() != 2 or labels.numel() != pr.shape[0]:
        raise BnnHipError("ece: probs must be [n, classes] and labels [n]")
    lb = labels.to(torch.int64).contiguous()
    edges = (C.c_double * len(bin_edges))(*[float(e) for e in bin_edges])
    ws = torch.empty(lib.bnn_ece_workspace_bytes() // 8, dtype=torch.float64, device=pr.device)
    out = torch.empty(1 + 3 * (len(bin_edges) - 1), dtype=torch.float32, device=pr.device)
    L.check(lib.bnn_ece(pr.data_ptr(), lb.data_ptr(), pr.shape[0], pr.shape[1], edges, len(bin_edges), ws.data_ptr(),
                        ws.numel() * 8, out.data_ptr(), _stream()), "bnn_ece")
    return out


def snr_db(mu: torch.Tensor, rho: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """F4: bnn_snr_db.  10 log10(|mu| / softplus(rho)) elementwise (fp32), shaped like mu."""
    lib = L.load()
    require_device(mu, rho)
    mu, rho = _f32c(mu, "mu"), _f32c(rho, "rho")
    if mu.numel() != rho.numel():
        raise BnnHipError("snr_db: mu and rho must have the same number of elements")
    if out is None:
        out = torch.empty_like(mu)
    L.check(lib.bnn_snr_db(mu.data_ptr(), rho.data_ptr(), mu.numel(), out.data_ptr(), _stream()), "bnn_snr_db")
    return out


def snr_prune_(mu: torch.Tensor, rho: torch.Tensor, threshold: float, kept: Optional[torch.Tensor] = None):
    """F4: bnn_snr_prune, IN PLACE on contiguous fp32 tensors: mu, rho *= (snr_db > threshold)."""
    lib = L.load()
    require_device(mu, rho)
    if mu.dtype != torch.float32 or rho.dtype != torch.float32 or not mu.is_contiguous() or not rho.is_contiguous() or \
            mu.numel() != rho.numel():
        raise BnnHipError("snr_prune_: contiguous float32 mu and rho of one size")
    L.check(lib.bnn_snr_prune(mu.data_ptr(), rho.data_ptr(), mu.numel(), float(threshold), _ptr(kept), _stream()),
            "bnn_snr_prune")


# ---------------------------------------------------------------------------------------------------------------- F5 bandit
def _typed(t: torch.Tensor, dtype: torch.dtype, name: str, numel: Optional[int] = None) -> torch.Tensor:
    require_device(t)
    if t.dtype != dtype or not t.is_contiguous():
        raise BnnHipError(f"{name} must be a contiguous {dtype} tensor")
    if numel is not None and t.numel() != numel:
        raise BnnHipError(f"{name} must have {numel} elements, got {t.numel()}")
    return t


def bandit_act_args(*, x, labels, rewards, oracle, outputs, n_samples: int, output_sample_stride: int, step, cur_index, rows,
                    actions, reward_out, regrets, counts, ring_index, ring_action, ring_reward, epsilon: float, seed: int,
                    indices=None, sample_counter=None, sample_counter_inc: int = 0) -> L.BanditActArgs:
    """The argument block of bnn_bandit_rows / bnn_bandit_act (include/bnn_hip.h F5), built once: the launches of a bandit
    step read everything that changes (t, i_t, the outputs) from device memory, so the same block serves every step.
    x [N, d] fp32, labels [N] int64, rewards [K, A, 3] fp32 (hi, lo, thr), oracle [K] fp32, outputs [S, A] (stride A) or
    [A] (stride 0), rows [A, d + A], actions / reward_out [max_steps], regrets [max_steps + 1] fp64, counts [K, A] int64,
    the ring [buffer_size] (int32 index, int32 action, fp32 reward), step / cur_index one int32 word each."""
    N, d = x.shape
    K, A = rewards.shape[0], rewards.shape[1]
    T = actions.numel()
    a = L.BanditActArgs()
    a.struct_bytes = C.sizeof(L.BanditActArgs)
    a.n_actions, a.n_labels, a.n_samples, a.output_sample_stride = A, K, int(n_samples), int(output_sample_stride)
    a.context_dim, a.n_contexts, a.buffer_size = d, N, ring_index.numel()
    a.max_steps, a.epsilon, a.seed = T, float(epsilon), int(seed) & 0xFFFFFFFFFFFFFFFF
    keep = [_typed(x, torch.float32, "x"), _typed(labels, torch.int64, "labels", N), _typed(rewards, torch.float32, "rewards", K * A * 3),
            _typed(oracle, torch.float32, "oracle", K), _typed(outputs, torch.float32, "outputs"),
            _typed(step, torch.int32, "step", 1), _typed(cur_index, torch.int32, "cur_index", 1),
            _typed(rows, torch.float32, "rows", A * (d + A)), _typed(actions, torch.int64, "actions"),
            _typed(reward_out, torch.float32, "reward_out", T), _typed(regrets, torch.float64, "regrets", T + 1),
            _typed(counts, torch.int64, "counts", K * A), _typed(ring_index, torch.int32, "ring_index"),
            _typed(ring_action, torch.int32, "ring_action", ring_index.numel()),
            _typed(ring_reward, torch.float32, "ring_reward", ring_index.numel())]
    (a.x, a.labels, a.rewards, a.oracle, a.outputs, a.step, a.cur_index, a.rows, a.actions, a.reward_out, a.regrets, a.counts,
     a.ring_index, a.ring_action, a.ring_reward) = (t.data_ptr() for t in keep)
    if outputs.numel() < (n_samples - 1) * output_sample_stride + A:
        raise BnnHipError("outputs is smaller than its samples and stride say")
    if indices is not None:
        keep.append(_typed(indices, torch.int64, "indices"))
        a.indices, a.n_indices = indices.data_ptr(), indices.numel()
    if sample_counter is not None:
        keep.append(_typed(sample_counter, torch.int32, "sample_counter", 1))
        a.sample_counter, a.sample_counter_inc = sample_counter.data_ptr(), int(sample_counter_inc) & 0xFFFFFFFF
    a._keep = keep
    return a


def bandit_rows(a: L.BanditActArgs):
    """bnn_bandit_rows: i_t (the index sequence's entry t, or drawn) and the A decision rows x[i_t] ++ one_hot(a)."""
    L.check(L.load().bnn_bandit_rows(C.byref(a), _stream()), "bnn_bandit_rows")


def bandit_act(a: L.BanditActArgs):
    """bnn_bandit_act: decision, reward, regret, counts and ring append of step t; advances the step word."""
    L.check(L.load().bnn_bandit_act(C.byref(a), _stream()), "bnn_bandit_act")


def bandit_replay_args(*, x, step, ring_index, ring_action, ring_reward, workspace, slab, targets, batch_size: int,
                       n_actions: int, seed: int, n_batches=None) -> L.BanditReplayArgs:
    """The argument block of bnn_bandit_replay: slab [num_batches, batch_size, d + A] fp32, targets [num_batches, batch_size]
    fp32, workspace int32 [buffer_size], n_batches (optional) one int32 word."""
    N, d = x.shape
    buf = ring_index.numel()
    nbm = slab.shape[0]
    a = L.BanditReplayArgs()
    a.struct_bytes = C.sizeof(L.BanditReplayArgs)
    a.batch_size, a.num_batches, a.buffer_size = int(batch_size), nbm, buf
    a.context_dim, a.n_actions, a.n_contexts, a.seed = d, int(n_actions), N, int(seed) & 0xFFFFFFFFFFFFFFFF
    keep = [_typed(step, torch.int32, "step", 1), _typed(x, torch.float32, "x"), _typed(ring_index, torch.int32, "ring_index"),
            _typed(ring_action, torch.int32, "ring_action", buf), _typed(ring_reward, torch.float32, "ring_reward", buf),
            _typed(workspace, torch.int32, "workspace", buf),
            _typed(slab, torch.float32, "slab", nbm * int(batch_size) * (d + int(n_actions))),
            _typed(targets, torch.float32, "targets", nbm * int(batch_size))]
    (a.step, a.x, a.ring_index, a.ring_action, a.ring_reward, a.workspace, a.slab, a.targets) = (t.data_ptr() for t in keep)
    if n_batches is not None:
        keep.append(_typed(n_batches, torch.int32, "n_batches", 1))
        a.n_batches = n_batches.data_ptr()
    a._keep = keep
    return a


def bandit_replay(a: L.BanditReplayArgs):
    """bnn_bandit_replay: the shuffled replay pool of the step just taken, gathered into the minibatch slab."""
    L.check(L.load().bnn_bandit_replay(C.byref(a), _stream()), "bnn_bandit_replay")


# ---------------------------------------------------------------------------------------------------------------- F6 groups
def _device_copy(arr, device) -> torch.Tensor:
    """The bytes of a ctypes array as a device uint8 tensor (the copy the group kernels read)."""
    return torch.frombuffer(bytearray(arr), dtype=torch.uint8).to(device)


def bandit_group_args(blocks: Sequence, device) -> L.BanditGroupArgs:
    """The argument block of bnn_bandit_*_group over G F5 blocks (all BanditActArgs or all BanditReplayArgs): the host
    array the entry validates and its device copy, made once here, that the kernels read."""
    if not blocks:
        raise BnnHipError("bandit_group_args: at least one block")
    cls = type(blocks[0])
    if cls not in (L.BanditActArgs, L.BanditReplayArgs) or any(type(b) is not cls for b in blocks):
        raise BnnHipError("bandit_group_args: blocks must all be BanditActArgs or all BanditReplayArgs")
    host = (cls * len(blocks))(*blocks)
    dev = _device_copy(host, device)
    g = L.BanditGroupArgs()
    g.struct_bytes = C.sizeof(L.BanditGroupArgs)
    g.n_agents, g.blocks_host, g.blocks, g.blocks_bytes = len(blocks), C.addressof(host), dev.data_ptr(), dev.numel()
    g._keep = (host, dev, [b._keep for b in blocks])
    return g


def bandit_rows_group(g: L.BanditGroupArgs):
    """bnn_bandit_rows_group: bnn_bandit_rows of every agent, one launch."""
    L.check(L.load().bnn_bandit_rows_group(C.byref(g), _stream()), "bnn_bandit_rows_group")


def bandit_act_group(g: L.BanditGroupArgs):
    """bnn_bandit_act_group: bnn_bandit_act of every agent, one launch."""
    L.check(L.load().bnn_bandit_act_group(C.byref(g), _stream()), "bnn_bandit_act_group")


def bandit_replay_group(g: L.BanditGroupArgs):
    """bnn_bandit_replay_group: bnn_bandit_replay of every agent, two launches."""
    L.check(L.load().bnn_bandit_replay_group(C.byref(g), _stream()), "bnn_bandit_replay_group")


def mlp_group_agent(*, params: Sequence[torch.Tensor], exp_avg=None, exp_avg_sq=None, step=None, lr=None, slab=None,
                    targets=None, n_batches=None, loss=None, rows=None, outputs=None) -> L.MlpGroupAgent:
    """One agent's block of bnn_mlp_group_*: params = (w1, b1, w2, b2, w3, b3) fp32 (nn.Linear layout), Adam's moments in the
    same order, step (int32 word), lr (fp32 word), slab [max_batches, batch, in], targets [max_batches * batch], n_batches
    (int32 word), loss (fp32 scalar) for training; rows [n_rows, in] and outputs [n_rows] for the decision forward."""
    a = L.MlpGroupAgent()
    keep = []
    a._named = dict(params=list(params), slab=slab, targets=targets, rows=rows, outputs=outputs)
    if len(params) != 6:
        raise BnnHipError("mlp_group_agent: six parameter tensors (w1, b1, w2, b2, w3, b3)")
    for f, ts in (("param", params), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
        if ts is None:
            continue
        if len(ts) != 6:
            raise BnnHipError(f"mlp_group_agent: six {f} tensors")
        arr = getattr(a, f)
        for i, t in enumerate(ts):
            keep.append(_typed(t, torch.float32, f"{f}[{i}]", params[i].numel()))
            arr[i] = t.data_ptr()
    for f, t, dt in (("step", step, torch.int32), ("lr", lr, torch.float32), ("slab", slab, torch.float32),
                     ("targets", targets, torch.float32), ("n_batches", n_batches, torch.int32), ("loss", loss, torch.float32),
                     ("rows", rows, torch.float32), ("outputs", outputs, torch.float32)):
        if t is not None:
            keep.append(_typed(t, dt, f))
            setattr(a, f, t.data_ptr())
    a._keep = keep
    return a


def mlp_group_args(agents: Sequence, *, in_features: int, hidden: int, device, batch: int = 0, max_batches: int = 0,
                   n_rows: int = 0, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0) -> L.MlpGroupArgs:
    """The argument block of bnn_mlp_group_fwd / _train over G agent blocks (mlp_group_agent), with the device copy of the
    blocks made once here.  Shapes are checked against the blocks' tensors: the training form (max_batches > 0) needs slab
    [max_batches, batch, in], the forward form (n_rows > 0) rows [n_rows, in]."""
    if not agents:
        raise BnnHipError("mlp_group_args: at least one agent")
    I, H = int(in_features), int(hidden)
    shapes = (H * I, H, H * H, H, H, 1)
    for ag in agents:
        if tuple(t.numel() for t in ag._named["params"]) != shapes:
            raise BnnHipError(f"mlp_group_args: the parameters must be an {I}-{H}-{H}-1 MLP's")
        named = ag._named
        if int(max_batches) and (named["slab"] is None or named["slab"].numel() != int(max_batches) * int(batch) * I or
                                          named["targets"] is None or named["targets"].numel() != int(max_batches) * int(batch)):
            raise BnnHipError("mlp_group_args: slab must be [max_batches, batch, in] and targets [max_batches, batch]")
        if int(n_rows) and (named["rows"] is None or named["rows"].numel() != int(n_rows) * I or named["outputs"] is None or
                                          named["outputs"].numel() != int(n_rows)):
            raise BnnHipError("mlp_group_args: rows must be [n_rows, in] and outputs [n_rows]")
    host = (L.MlpGroupAgent * len(agents))(*agents)
    dev = _device_copy(host, device)
    a = L.MlpGroupArgs()
    a.struct_bytes = C.sizeof(L.MlpGroupArgs)
    a.n_agents, a.in_features, a.hidden, a.out_features = len(agents), int(in_features), int(hidden), 1
    a.batch, a.max_batches, a.n_rows = int(batch), int(max_batches), int(n_rows)
    a.beta1, a.beta2, a.eps, a.weight_decay = float(betas[0]), float(betas[1]), float(eps), float(weight_decay)
    a.agents_host, a.agents, a.agents_bytes = C.addressof(host), dev.data_ptr(), dev.numel()
    a._keep = (host, dev, [ag._keep for ag in agents])
    return a


def mlp_group_fwd(a: L.MlpGroupArgs):
    """bnn_mlp_group_fwd: every agent's forward of its rows, one launch."""
    L.check(L.load().bnn_mlp_group_fwd(C.byref(a), _stream()), "bnn_mlp_group_fwd")


def mlp_group_train(a: L.MlpGroupArgs):
    """bnn_mlp_group_train: every agent's nb minibatch steps (forward, mse_loss(sum), backward, Adam), one launch."""
    L.check(L.load().bnn_mlp_group_train(C.byref(a), _stream()), "bnn_mlp_group_train")


# ---------------------------------------------------------------------------------------------------------------- F7 groups
def bbb_group_workspace_bytes(in_features: int, hidden: int) -> int:
    """bnn_bbb_group_workspace_bytes: bytes of one agent's workspace (0 outside the limits)."""
    return int(L.load().bnn_bbb_group_workspace_bytes(int(in_features), int(hidden)))


def bbb_group_agent(*, params: Sequence[torch.Tensor], workspace: torch.Tensor, eps_seed: int, exp_avg=None, exp_avg_sq=None,
                    step=None, lr=None, slab=None, targets=None, n_batches=None, loss_info=None, rows=None, outputs=None,
                    sample_counter=None, eps_mode: int = L.EPS_PHILOX) -> L.BbbGroupAgent:
    """One agent's block of bnn_bbb_group_*: params = the twelve tensors of networks.BayesianNetwork.parameters()
    ((weight_mu, weight_rho, bias_mu, bias_rho) of l1, l2, l3; fp32), Adam's moments in the same order, step (int32 word), lr
    (fp32 word), slab [max_batches, batch, in], targets [max_batches * batch], n_batches (int32 word), loss_info (fp32 [4]),
    sample_counter (int32 word) for training; rows [n_rows, in], outputs and eps_mode (L.EPS_PHILOX: a draw per sample,
    L.EPS_ZERO: w = mu) for the decision forward; workspace (fp32, bbb_group_workspace_bytes) and eps_seed for both."""
    a = L.BbbGroupAgent()
    keep = []
    a._named = dict(params=list(params), slab=slab, targets=targets, rows=rows, outputs=outputs, workspace=workspace)
    if len(params) != 12:
        raise BnnHipError("bbb_group_agent: twelve parameter tensors ((weight_mu, weight_rho, bias_mu, bias_rho) x 3 layers)")
    for f, ts in (("param", params), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
        if ts is None:
            continue
        if len(ts) != 12:
            raise BnnHipError(f"bbb_group_agent: twelve {f} tensors")
        arr = getattr(a, f)
        for i, t in enumerate(ts):
            keep.append(_typed(t, torch.float32, f"{f}[{i}]", params[i].numel()))
            arr[i] = t.data_ptr()
    for f, t, dt in (("step", step, torch.int32), ("lr", lr, torch.float32), ("slab", slab, torch.float32),
                     ("targets", targets, torch.float32), ("n_batches", n_batches, torch.int32),
                     ("loss_info", loss_info, torch.float32), ("rows", rows, torch.float32), ("outputs", outputs, torch.float32),
                     ("sample_counter", sample_counter, torch.int32), ("workspace", workspace, torch.float32)):
        if t is not None:
            keep.append(_typed(t, dt, f))
            setattr(a, f, t.data_ptr())
    if loss_info is not None and loss_info.numel() != 4:
        raise BnnHipError("bbb_group_agent: loss_info must have 4 elements (loss, log_p, log_q, nll)")
    if eps_mode not in (L.EPS_PHILOX, L.EPS_ZERO):
        raise BnnHipError("bbb_group_agent: eps_mode must be EPS_PHILOX or EPS_ZERO")
    a.eps_seed, a.eps_mode = int(eps_seed) & 0xFFFFFFFFFFFFFFFF, int(eps_mode)
    a._keep = keep
    return a


def bbb_group_args(agents: Sequence, *, in_features: int, hidden: int, n_samples: int, device, prior: Optional[PriorSpec] = None,
                   batch: int = 0, max_batches: int = 0, n_rows: int = 0, kl_weights: Sequence[float] = (),
                   betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0) -> L.BbbGroupArgs:
    """The argument block of bnn_bbb_group_fwd / _train over G agent blocks (bbb_group_agent), with the device copy of the
    blocks made once here.  The training form (max_batches > 0) needs slab [max_batches, batch, in], the prior and
    kl_weights[j], the KL weight of minibatch j < max_batches (rounded to fp32 here); the forward form (n_rows > 0) rows
    [n_rows, in] and outputs of n_samples * n_rows elements (n_rows for an EPS_ZERO agent)."""
    if not agents:
        raise BnnHipError("bbb_group_args: at least one agent")
    I, H, S = int(in_features), int(hidden), int(n_samples)
    shapes = (H * I, H * I, H, H, H * H, H * H, H, H, H, H, 1, 1)
    if int(max_batches) > L.MLP_GROUP_MAX_BATCHES or len(kl_weights) > L.MLP_GROUP_MAX_BATCHES:
        raise BnnHipError(f"bbb_group_args: at most {L.MLP_GROUP_MAX_BATCHES} minibatches per update")
    if int(max_batches) and len(kl_weights) < int(max_batches):
        raise BnnHipError("bbb_group_args: one KL weight per minibatch of the slab")
    need = bbb_group_workspace_bytes(I, H)
    ws_bytes = min(ag._named["workspace"].numel() * 4 for ag in agents)
    for ag in agents:
        named = ag._named
        if tuple(t.numel() for t in named["params"]) != shapes:
            raise BnnHipError(f"bbb_group_args: the parameters must be an {I}-{H}-{H}-1 BayesianNetwork's")
        if int(max_batches) and (named["slab"] is None or named["slab"].numel() != int(max_batches) * int(batch) * I or
                                          named["targets"] is None or named["targets"].numel() != int(max_batches) * int(batch)):
            raise BnnHipError("bbb_group_args: slab must be [max_batches, batch, in] and targets [max_batches, batch]")
        if int(n_rows):
            want = int(n_rows) * (1 if ag.eps_mode == L.EPS_ZERO else S)
            if named["rows"] is None or named["rows"].numel() != int(n_rows) * I or named["outputs"] is None or \
                    named["outputs"].numel() < want:
                raise BnnHipError("bbb_group_args: rows must be [n_rows, in] and outputs [n_samples, n_rows]")
    host = (L.BbbGroupAgent * len(agents))(*agents)
    dev = _device_copy(host, device)
    a = L.BbbGroupArgs()
    a.struct_bytes = C.sizeof(L.BbbGroupArgs)
    a.n_agents, a.in_features, a.hidden, a.out_features = len(agents), I, H, 1
    a.batch, a.max_batches, a.n_rows, a.n_samples = int(batch), int(max_batches), int(n_rows), S
    a.prior = (prior if prior is not None else PriorSpec()).c()
    a.beta1, a.beta2, a.eps, a.weight_decay = float(betas[0]), float(betas[1]), float(eps), float(weight_decay)
    for j, b in enumerate(kl_weights):
        a.beta[j] = float(b)
    a.workspace_bytes = ws_bytes
    a.agents_host, a.agents, a.agents_bytes = C.addressof(host), dev.data_ptr(), dev.numel()
    a._keep = (host, dev, [ag._keep for ag in agents])
    return a


def bbb_group_fwd(a: L.BbbGroupArgs):
    """bnn_bbb_group_fwd: every agent's forward of its rows under its posterior draws (or w = mu), one launch."""
    L.check(L.load().bnn_bbb_group_fwd(C.byref(a), _stream()), "bnn_bbb_group_fwd")


def bbb_group_train(a: L.BbbGroupArgs):
    """bnn_bbb_group_train: every agent's nb minibatch steps (BBB forward, ELBO, backward through mu and rho, Adam), one launch."""
    L.check(L.load().bnn_bbb_group_train(C.byref(a), _stream()), "bnn_bbb_group_train")


def dropout_params(p: float) -> tuple:
    """(thr, scale) of the kind-3 dropout map (include/bnn_hip.h) for a drop probability p in [0, 1), in fp64 as the
    library forms them.  Raises BnnHipError outside that range."""
    p = float(p)
    if not 0.0 <= p < 1.0:                               # (NaN fails)
        raise BnnHipError(f"dropout probability must lie in [0, 1), got {p}")
    return min(math.floor(p * 2.0 ** 32), 2 ** 32 - 1), C.c_float(1.0 / (1.0 - p)).value


def dropout_mask(seed: int, layer_id: int, sample_offset: int, n_samples: int, rows: int, cols: int, p: float,
                 device) -> torch.Tensor:
    """The kind-3 dropout stream of layer `layer_id`, materialised (bnn_dropout_mask): float32[n_samples, rows, cols]
    holding 1 / (1 - p) where an element is kept and 0 where it is dropped."""
    lib = L.load()
    dropout_params(p)
    if torch.device(device).type != "cuda":
        raise BnnHipError("bnn_hip.dropout_mask needs a ROCm device")
    mask = torch.empty((n_samples, rows, cols), dtype=torch.float32, device=device)
    L.check(lib.bnn_dropout_mask(mask.data_ptr(), seed & 0xFFFFFFFFFFFFFFFF, int(layer_id), sample_offset & 0xFFFFFFFF,
                                 n_samples, rows, cols, float(p), _stream()), "bnn_dropout_mask")
    return mask


def _dense_build(x, w, b, *, n_samples: int, math_mode: int, relu: bool, drop_p: float, layer_id: int, seed: int,
                 sample_offset: int = 0, sample_counter=None, sample_counter_inc: int = 0, y_dtype=torch.float32, out=None):
    """(args, keep-alive, y) of one bnn_dense_fwd launch: x [B, in] (shared by the samples) or [S, B, in]."""
    require_device(x, w, b, out, sample_counter)
    dropout_params(drop_p)
    w = _f32c(w, "weight")
    b = None if b is None else _f32c(b, "bias")
    if x.dim() == 2:
        shared, B, K = 1, x.shape[0], x.shape[1]
    elif x.dim() == 3 and x.shape[0] == n_samples:
        shared, B, K = 0, x.shape[1], x.shape[2]
    else:
        raise BnnHipError(f"dense_fwd: x must be [batch, in] or [{n_samples}, batch, in], got {tuple(x.shape)}")
    x = x if x.is_contiguous() else x.contiguous()
    N = w.shape[0]
    if w.dim() != 2 or w.shape[1] != K or (b is not None and tuple(b.shape) != (N,)):
        raise BnnHipError(f"dense_fwd: weight {tuple(w.shape)} / bias do not fit x of {K} features")
    if out is None:
        out = torch.empty((n_samples, B, N), dtype=y_dtype, device=x.device)
    elif tuple(out.shape) != (n_samples, B, N) or not out.is_contiguous():
        raise BnnHipError(f"dense_fwd: out must be a contiguous [{n_samples}, {B}, {N}] tensor")
    if sample_counter is not None and (sample_counter.dtype != torch.int32 or sample_counter.numel() != 1):
        raise BnnHipError("dense_fwd: sample_counter must be a one-element int32 device tensor")
    a = L.DenseFwdArgs()
    a.struct_bytes = C.sizeof(L.DenseFwdArgs)
    a.n_samples, a.batch, a.in_features, a.out_features = int(n_samples), B, K, N
    a.x_shared, a.x, a.x_dtype = shared, x.data_ptr(), _dt(x)
    a.math = int(math_mode)
    a.w, a.b = w.data_ptr(), _ptr(b)
    a.relu, a.layer_id, a.drop_p = int(bool(relu)), int(layer_id), float(drop_p)
    a.seed, a.sample_offset = int(seed) & 0xFFFFFFFFFFFFFFFF, int(sample_offset) & 0xFFFFFFFF
    a.sample_counter, a.sample_counter_inc = _ptr(sample_counter), int(sample_counter_inc)
    a.y, a.y_dtype = out.data_ptr(), _dt(out)
    return a, (x, w, b, out, sample_counter), out


def dense_fwd(x, w, b, **kw) -> torch.Tensor:
    """K5: y[s] = drop_s(act(x[s'] . w^T + b)) for n_samples MC-dropout samples in one launch (bnn_dense_fwd).  The kind-3
    mask of `layer_id` at global sample index sample_offset + *sample_counter + s; drop_p = 0 applies none."""
    lib = L.load()
    a, keep, y = _dense_build(x, w, b, **kw)
    a._keep = keep                    # (the structure owns what its pointers refer to: a recorded launch list replays it)
    L.check(lib.bnn_dense_fwd(C.byref(a), _stream()), "bnn_dense_fwd")
    return y


def dense_plan(x, w, b, **kw) -> dict:
    """What bnn_dense_fwd would launch for these arguments (bnn_dense_plan)."""
    lib = L.load()
    a, _, _ = _dense_build(x, w, b, **kw)
    pl = L.Plan()
    L.check(lib.bnn_dense_plan(C.byref(a), C.byref(pl)), "bnn_dense_plan")
    return _plan_dict(pl)


def dense_loss(logits, target, mode: str, *, grad_scale: float = 1.0, loss=None, g_logits=None):
    """K6 bnn_dense_loss: (loss 0-dim, g_logits [B, C]) of cross_entropy(logits, target, reduction='sum') (classification,
    int64 labels [B]) or mse_loss(logits, target, reduction='sum') (regression, fp32 target of B * C elements), the
    gradient times grad_scale, in one launch.  An out-of-range label gives a NaN loss and NaN gradient row."""
    lib = L.load()
    require_device(logits, target, loss, g_logits)
    logits = _f32c(logits, "logits")
    if logits.dim() != 2:
        raise BnnHipError(f"dense_loss: logits must be [batch, classes], got {tuple(logits.shape)}")
    B, Cc = logits.shape
    if mode == "classification":
        if target.dtype != torch.int64 or target.numel() != B:
            raise BnnHipError("dense_loss: classification targets must be int64 labels, one per row")
        lm = L.NLL_CLASSIFICATION
    elif mode == "regression":
        if target.dtype != torch.float32 or target.numel() != B * Cc:
            raise BnnHipError(f"dense_loss: regression targets must be float32 with {B * Cc} elements")
        lm = L.NLL_REGRESSION
    else:
        raise BnnHipError(f"dense_loss: unknown mode {mode!r}")
    target = target if target.is_contiguous() else target.contiguous()
    if loss is None:
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
    if g_logits is None:
        g_logits = torch.empty_like(logits)
    elif tuple(g_logits.shape) != (B, Cc) or g_logits.dtype != torch.float32 or not g_logits.is_contiguous():
        raise BnnHipError("dense_loss: g_logits must be a contiguous float32 tensor of the logits' shape")
    a = L.DenseLossArgs()
    a.struct_bytes = C.sizeof(L.DenseLossArgs)
    a.batch, a.classes, a.loss_mode = B, Cc, lm
    a.logits, a.target, a.grad_scale = logits.data_ptr(), target.data_ptr(), float(grad_scale)
    a.loss, a.g_logits = loss.data_ptr(), g_logits.data_ptr()
    L.check(lib.bnn_dense_loss(C.byref(a), _stream()), "bnn_dense_loss")
    return loss, g_logits


def dense_bwd(x, gy, w, *, g_w, g_b=None, g_x=None, y=None, y_scale: float = 1.0, gx_mask: bool = False,
              gx_scale: float = 1.0, math_mode: int = L.MATH_F32):
    """K6 bnn_dense_bwd: the backward of one Linear -> [ReLU] -> [Dropout] group into the given buffers.  gz = gy, or
    (y > 0 ? gy * y_scale : 0) with the saved output y; g_w = gz^T x, g_b = colsum(gz), g_x = gz W (optional) times
    (x > 0 ? gx_scale : 0) when gx_mask.  All fp32 contiguous device tensors."""
    lib = L.load()
    require_device(x, gy, w, g_w, g_b, g_x, y)
    B, K = x.shape
    N = w.shape[0]
    shapes = ((x, (B, K)), (gy, (B, N)), (w, (N, K)), (g_w, (N, K)), (g_b, (N,)), (g_x, (B, K)), (y, (B, N)))
    for t, shp in shapes:
        if t is not None and (tuple(t.shape) != shp or t.dtype != torch.float32 or not t.is_contiguous()):
            raise BnnHipError(f"dense_bwd: expected a contiguous float32 tensor of shape {shp}, got {tuple(t.shape)} {t.dtype}")
    a = L.DenseBwdArgs()
    a.struct_bytes = C.sizeof(L.DenseBwdArgs)
    a.batch, a.in_features, a.out_features = B, K, N
    a.math, a.gx_mask = _exact_unless_bf16(math_mode), int(bool(gx_mask))
    a.x, a.gy, a.y, a.w = x.data_ptr(), gy.data_ptr(), _ptr(y), w.data_ptr()
    a.y_scale, a.gx_scale = float(y_scale), float(gx_scale)
    a.g_w, a.g_b, a.g_x = g_w.data_ptr(), _ptr(g_b), _ptr(g_x)
    L.check(lib.bnn_dense_bwd(C.byref(a), _stream()), "bnn_dense_bwd")


def sgd_step(params, grads, *, lr: float, weight_decay: float = 0.0, lr_device=None):
    """K6 bnn_sgd_step: p -= lr * (g + weight_decay * p) over lists of fp32 tensors, 16 per launch; `lr_device` (device
    float[1]) overrides lr."""
    lib = L.load()
    n = len(params)
    require_device(lr_device)
    for lo in range(0, n, L.SGD_MAX_TENSORS):
        hi = min(n, lo + L.SGD_MAX_TENSORS)
        a = L.SgdArgs()
        a.struct_bytes = C.sizeof(L.SgdArgs)
        a.n_tensors = hi - lo
        for j in range(lo, hi):
            p, g = params[j], grads[j]
            require_device(p, g)
            if p.dtype != torch.float32 or g.dtype != torch.float32 or not p.is_contiguous() or not g.is_contiguous() or \
                    g.numel() != p.numel():
                raise BnnHipError("sgd_step: parameters and gradients must be contiguous float32 of one size")
            a.param[j - lo], a.grad[j - lo], a.numel[j - lo] = p.data_ptr(), g.data_ptr(), p.numel()
        a.lr, a.weight_decay, a.lr_device = float(lr), float(weight_decay), _ptr(lr_device)
        L.check(lib.bnn_sgd_step(C.byref(a), _stream()), "bnn_sgd_step")


# ---------------------------------------------------------------------------------------------------------------- F8 epochs
def epoch_perm_args(*, n_rows: int, seed: int, epoch, order) -> L.EpochPermArgs:
    """The argument block of bnn_epoch_permutation: `epoch` one int32 device word, `order` int32 [n_rows]."""
    a = L.EpochPermArgs()
    a.struct_bytes = C.sizeof(L.EpochPermArgs)
    a.n_rows, a.seed = int(n_rows), int(seed) & 0xFFFFFFFFFFFFFFFF
    keep = [_typed(epoch, torch.int32, "epoch", 1), _typed(order, torch.int32, "order", int(n_rows))]
    a.epoch, a.order = (t.data_ptr() for t in keep)
    a._keep = keep
    return a


def epoch_permutation(a: L.EpochPermArgs):
    """bnn_epoch_permutation: the positions sorted by (Philox key, position) into `order`, one launch."""
    L.check(L.load().bnn_epoch_permutation(C.byref(a), _stream()), "bnn_epoch_permutation")


def epoch_stage_args(*, x, targets, batch_size: int, num_batches: int, batch_index, epoch, ticket, x_out, targets_out,
                     order=None, x_bf16_out=None, beta_table=None, beta=None, loss_src=(), loss_history=None) -> L.EpochStageArgs:
    """The argument block of bnn_epoch_stage (include/bnn_hip.h F8), built once per destination: the launch reads the
    minibatch number from `batch_index`, so the same block serves every minibatch of every epoch.  x [N, d] float32 or
    uint8, targets [N] int64 or [N, k] float32; x_out float32 and x_bf16_out bfloat16 of B * d elements, targets_out of B
    (* k); batch_index / epoch / ticket one int32 word each; loss_src up to 4 float32 device words (views are fine) filed
    into loss_history [num_batches, len(loss_src)] by the NEXT minibatch's launch."""
    require_device(x, targets)
    if x.dim() != 2 or x.dtype not in (torch.float32, torch.uint8) or not x.is_contiguous():
        raise BnnHipError("epoch_stage: x must be a contiguous [N, d] float32 or uint8 tensor")
    N, d = x.shape
    B, M = int(batch_size), int(num_batches)
    if targets.dtype == torch.int64:
        k = 0
        _typed(targets, torch.int64, "targets", N)
    else:
        if targets.dim() != 2:
            raise BnnHipError("epoch_stage: float32 targets must be [N, k]")
        k = int(targets.shape[1])
        _typed(targets, torch.float32, "targets", N * k)
    a = L.EpochStageArgs()
    a.struct_bytes = C.sizeof(L.EpochStageArgs)
    a.n_rows, a.row_dim, a.batch_size, a.num_batches = N, d, B, M
    a.x_dtype, a.target_dim = (L.EPOCH_X_U8 if x.dtype == torch.uint8 else L.EPOCH_X_F32), k
    keep = [x, targets, _typed(batch_index, torch.int32, "batch_index", 1), _typed(epoch, torch.int32, "epoch", 1),
            _typed(ticket, torch.int32, "ticket", 1), _typed(x_out, torch.float32, "x_out", B * d),
            _typed(targets_out, targets.dtype, "targets_out", B * max(k, 1))]
    a.x, a.targets, a.batch_index, a.epoch, a.ticket, a.x_out, a.targets_out = (t.data_ptr() for t in keep)
    if order is not None:
        keep.append(_typed(order, torch.int32, "order", N))
        a.order = order.data_ptr()
    if x_bf16_out is not None:
        keep.append(_typed(x_bf16_out, torch.bfloat16, "x_bf16_out", B * d))
        a.x_bf16_out = x_bf16_out.data_ptr()
    if beta_table is not None:
        keep += [_typed(beta_table, torch.float32, "beta_table", M), _typed(beta, torch.float32, "beta", 1)]
        a.beta_table, a.beta = beta_table.data_ptr(), beta.data_ptr()
    if loss_history is not None:
        if not 1 <= len(loss_src) <= L.EPOCH_MAX_LOSS_COLS:
            raise BnnHipError(f"epoch_stage: 1 to {L.EPOCH_MAX_LOSS_COLS} loss words")
        a.loss_cols = len(loss_src)
        for c, w in enumerate(loss_src):
            keep.append(_typed(w, torch.float32, "loss_src", 1))
            a.loss_src[c] = w.data_ptr()
        keep.append(_typed(loss_history, torch.float32, "loss_history", M * len(loss_src)))
        a.loss_history = loss_history.data_ptr()
    a._keep = keep
    return a


def epoch_stage(a: L.EpochStageArgs):
    """bnn_epoch_stage: gather, cast and target copy of minibatch *batch_index, beta lookup, loss filing; advances the
    minibatch word (and the epoch word after the last minibatch)."""
    L.check(L.load().bnn_epoch_stage(C.byref(a), _stream()), "bnn_epoch_stage")


# ---------------------------------------------------------------------------------------------------------------- F9 pruning sweep
def snr_select(segments, fractions, out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bnn_snr_select: the np.percentile thresholds (float64 [P], on the device, no host read) of the fp32 SNR values held
    in `segments` (a list of device tensors, never concatenated) at the drop `fractions` (host floats in [0, 1], any order)."""
    lib = L.load()
    segs = [_f32c(s, "snr").reshape(-1) for s in segments]
    require_device(*segs)
    fr = [float(f) for f in fractions]
    if not 1 <= len(segs) <= L.PRUNE_MAX_SEGMENTS or not 1 <= len(fr) <= L.PRUNE_MAX_LEVELS:
        raise BnnHipError(f"snr_select: 1 to {L.PRUNE_MAX_SEGMENTS} segments and 1 to {L.PRUNE_MAX_LEVELS} levels")
    dev = segs[0].device
    if out is None:
        out = torch.empty(len(fr), dtype=torch.float64, device=dev)
    if workspace is None:
        workspace = torch.empty(lib.bnn_snr_select_workspace_bytes() // 8 + 1, dtype=torch.int64, device=dev)
    a = L.SnrSelectArgs()
    a.struct_bytes = C.sizeof(L.SnrSelectArgs)
    a.n_segments, a.n_levels = len(segs), len(fr)
    for i, s in enumerate(segs):
        a.snr[i], a.n[i] = s.data_ptr(), s.numel()
    for i, f in enumerate(fr):
        a.fraction[i] = f
    a.workspace, a.workspace_bytes, a.thresholds = workspace.data_ptr(), workspace.numel() * 8, out.data_ptr()
    L.check(lib.bnn_snr_select(C.byref(a), _stream()), "bnn_snr_select")
    return out


def prune_codes(mu: torch.Tensor, rho: torch.Tensor, thresholds: torch.Tensor, code: torch.Tensor, mu_out: torch.Tensor,
                kept: torch.Tensor, *, out_features: int, in_features: int, transposed: bool):
    """bnn_prune_codes: the level codes and the matmul-ready mu of one parameter tensor into the canonical [out, ld] images
    `code` (uint8) and `mu_out` (float32 or bfloat16); kept (int64 [P]) += the survivors of each level."""
    require_device(mu, rho, thresholds, code, mu_out, kept)
    mu, rho = _f32c(mu, "mu"), _f32c(rho, "rho")
    if mu.numel() != out_features * in_features or rho.numel() != mu.numel():
        raise BnnHipError("prune_codes: mu and rho must hold out_features * in_features elements")
    if code.dtype != torch.uint8 or code.dim() != 2 or code.shape != mu_out.shape or not code.is_contiguous() or \
            not mu_out.is_contiguous() or code.shape[0] < out_features:
        raise BnnHipError("prune_codes: code (uint8) and mu_out must be contiguous [>= out_features, ld] images of one shape")
    if thresholds.dtype != torch.float64 or kept.dtype != torch.int64 or kept.numel() != thresholds.numel():
        raise BnnHipError("prune_codes: thresholds float64 [P], kept int64 [P]")
    a = L.PruneCodesArgs()
    a.struct_bytes = C.sizeof(L.PruneCodesArgs)
    a.out_features, a.in_features, a.ld, a.transposed = int(out_features), int(in_features), code.shape[1], int(bool(transposed))
    a.n_levels, a.mu_dtype = thresholds.numel(), _dt(mu_out)
    a.mu, a.rho, a.thresholds = mu.data_ptr(), rho.data_ptr(), thresholds.data_ptr()
    a.code, a.mu_out, a.kept = code.data_ptr(), mu_out.data_ptr(), kept.data_ptr()
    L.check(L.load().bnn_prune_codes(C.byref(a), _stream()), "bnn_prune_codes")


def pruned_fwd_args(*, x: torch.Tensor, mu: torch.Tensor, code: torch.Tensor, b: Optional[torch.Tensor],
                    bcode: Optional[torch.Tensor], y: torch.Tensor, n_levels: int, rows: int, in_features: int,
                    out_features: int, math_mode: int, relu: bool, x_shared: bool) -> L.PrunedFwdArgs:
    """The argument block of bnn_pruned_fwd for one layer: x [rows, ldx] (shared) or [P, rows, ldx], y [P, rows, ldy], the
    canonical mu / code images [round_up(out, 64), ld]."""
    require_device(x, mu, code, y, b, bcode)
    if not (x.is_contiguous() and y.is_contiguous() and mu.is_contiguous() and code.is_contiguous()):
        raise BnnHipError("pruned_fwd: contiguous tensors")
    if mu.shape != code.shape or mu.shape[0] < -(-out_features // 64) * 64 or code.dtype != torch.uint8:
        raise BnnHipError("pruned_fwd: mu and code must be [round_up(out_features, 64), ld] images of one shape")
    if x.numel() != (1 if x_shared else n_levels) * rows * x.shape[-1] or y.numel() != n_levels * rows * y.shape[-1]:
        raise BnnHipError("pruned_fwd: x must be [rows, ldx] or [P, rows, ldx] and y [P, rows, ldy]")
    a = L.PrunedFwdArgs()
    a.struct_bytes = C.sizeof(L.PrunedFwdArgs)
    a.n_levels, a.rows, a.in_features, a.out_features = int(n_levels), int(rows), int(in_features), int(out_features)
    a.math, a.relu, a.x_shared = int(math_mode), int(bool(relu)), int(bool(x_shared))
    a.x_dtype, a.y_dtype, a.ldx, a.ldy, a.ld = _dt(x), _dt(y), x.shape[-1], y.shape[-1], mu.shape[1]
    a.x, a.mu, a.code, a.b, a.bcode, a.y = x.data_ptr(), mu.data_ptr(), code.data_ptr(), _ptr(b), _ptr(bcode), y.data_ptr()
    return a


def pruned_fwd(a: L.PrunedFwdArgs):
    L.check(L.load().bnn_pruned_fwd(C.byref(a), _stream()), "bnn_pruned_fwd")


def prune_sweep_tail(logits: torch.Tensor, target: torch.Tensor, *, mode: int, probs: Optional[torch.Tensor],
                     correct: Optional[torch.Tensor], loss: torch.Tensor, row0: int, n_total: int):
    """bnn_prune_sweep_tail over the logits [P, rows, classes] of one minibatch (rows row0 .. of a data set of n_total)."""
    require_device(logits, target, probs, correct, loss)
    P, rows, classes = logits.shape
    if logits.dtype != torch.float32 or not logits.is_contiguous() or not target.is_contiguous():
        raise BnnHipError("prune_sweep_tail: contiguous float32 logits [P, rows, classes] and a contiguous target")
    if mode == L.NLL_CLASSIFICATION:
        if target.dtype != torch.int64 or target.numel() != rows:
            raise BnnHipError("prune_sweep_tail: int64 labels [rows]")
        if probs is None or probs.dtype != torch.float32 or not probs.is_contiguous() or probs.numel() != P * n_total * classes or \
                correct is None or correct.dtype != torch.int64 or correct.numel() != P:
            raise BnnHipError("prune_sweep_tail: probs float32 [P, n_total, classes] and correct int64 [P]")
    elif target.dtype != torch.float32 or target.numel() != rows * classes:
        raise BnnHipError("prune_sweep_tail: float32 targets [rows, classes]")
    if loss.dtype != torch.float64 or loss.numel() != P:
        raise BnnHipError("prune_sweep_tail: loss float64 [P]")
    a = L.PruneTailArgs()
    a.struct_bytes = C.sizeof(L.PruneTailArgs)
    a.mode, a.n_levels, a.rows, a.classes, a.n_total, a.row0 = int(mode), P, rows, classes, int(n_total), int(row0)
    a.logits, a.target, a.probs, a.correct, a.loss = logits.data_ptr(), target.data_ptr(), _ptr(probs), _ptr(correct), loss.data_ptr()
    L.check(L.load().bnn_prune_sweep_tail(C.byref(a), _stream()), "bnn_prune_sweep_tail")


# ---------------------------------------------------------------------------------------------------------------- F10 active learning
def acquire_topk_workspace(device) -> torch.Tensor:
    """bnn_acquire_topk's workspace (any contents; 8-byte aligned)."""
    return torch.empty(L.load().bnn_acquire_topk_workspace_bytes() // 8 + 1, dtype=torch.int64, device=device)


def acquire_topk_args(*, scores, candidate, k: int, selected, labelled, n_labelled, n_selected=None,
                      workspace=None) -> L.AcquireTopkArgs:
    """The argument block of bnn_acquire_topk (include/bnn_hip.h F10): scores float32 [N], candidate uint8 [N], selected
    int32 [k], labelled int32 [N], n_labelled / n_selected one int32 device word each."""
    N = scores.numel()
    keep = [_typed(scores, torch.float32, "scores"), _typed(candidate, torch.uint8, "candidate", N),
            _typed(selected, torch.int32, "selected", int(k)), _typed(labelled, torch.int32, "labelled", N),
            _typed(n_labelled, torch.int32, "n_labelled", 1)]
    a = L.AcquireTopkArgs()
    a.struct_bytes = C.sizeof(L.AcquireTopkArgs)
    a.n_rows, a.k = N, int(k)
    a.scores, a.candidate, a.selected, a.labelled, a.n_labelled = (t.data_ptr() for t in keep)
    if n_selected is not None:
        keep.append(_typed(n_selected, torch.int32, "n_selected", 1))
        a.n_selected = n_selected.data_ptr()
    if workspace is None:
        workspace = acquire_topk_workspace(scores.device)
    require_device(workspace)
    keep.append(workspace)
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    a._keep = keep
    return a


def acquire_topk(a: L.AcquireTopkArgs):
    """bnn_acquire_topk: the first k candidates by (score descending, row ascending, NaN last) into `selected`; the mask,
    the labelled list and its count word follow on the device."""
    L.check(L.load().bnn_acquire_topk(C.byref(a), _stream()), "bnn_acquire_topk")


def acquire_compose(labelled: torch.Tensor, perm: torch.Tensor, order: torch.Tensor, n: int):
    """bnn_acquire_compose: order[i] = labelled[perm[i]], i < n."""
    for t, name in ((labelled, "labelled"), (perm, "perm"), (order, "order")):
        _typed(t, torch.int32, name)
        if t.numel() < int(n):
            raise BnnHipError(f"acquire_compose: {name} must hold at least {int(n)} entries")
    L.check(L.load().bnn_acquire_compose(labelled.data_ptr(), perm.data_ptr(), order.data_ptr(), int(n), _stream()),
            "bnn_acquire_compose")


def acquire_random(scores: torch.Tensor, seed: int, round: int) -> torch.Tensor:
    """bnn_acquire_random: one Philox uniform in [0, 1) per row, counter (row >> 2, round, 3, 1), word row & 3."""
    _typed(scores, torch.float32, "scores")
    L.check(L.load().bnn_acquire_random(scores.data_ptr(), scores.numel(), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                        int(round) & 0xFFFFFFFF, _stream()), "bnn_acquire_random")
    return scores


# ---------------------------------------------------------------------------------------------------------------- F11 posterior statistics
def hist_edges(edges):
    """The bin-edge table of bnn_param_hist as a float64 numpy array: 2 .. HIST_MAX_EDGES finite, strictly increasing edges."""
    import numpy as np
    e = np.ascontiguousarray(np.asarray(edges, dtype=np.float64).reshape(-1))
    if not 2 <= e.size <= L.HIST_MAX_EDGES:
        raise BnnHipError(f"param_hist: 2 to {L.HIST_MAX_EDGES} bin edges, got {e.size}")
    if not (np.all(np.isfinite(e)) and np.all(e[1:] > e[:-1])):
        raise BnnHipError("param_hist: the bin edges must be finite and strictly increasing")
    return e


def _hist_f32(t, name: str) -> torch.Tensor:
    if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_contiguous():
        raise BnnHipError(f"param_hist: {name} must be a contiguous float32 tensor (tensors are neither copied nor padded)")
    return t


def param_hist_args(jobs: Sequence[dict], edges, *, records: Optional[torch.Tensor] = None,
                    workspace: Optional[torch.Tensor] = None) -> L.ParamHistArgs:
    """The argument block of bnn_param_hist (include/bnn_hip.h F11).  `jobs`: dicts with kind (L.HIST_*), src0, and by kind
    src1 (SNR_DB, SAMPLE), seed / tensor_id / sample (SAMPLE; rows x cols is src0's shape, a vector a single row), values_out
    (optional float32 [n]).  `edges`: the host table.  `records` (int64 [n_jobs, hist_record_bytes / 8]) and `workspace` are
    allocated when not given; the block keeps them as .records / .workspace and the device table as .edges_device."""
    e = hist_edges(edges)
    if not 1 <= len(jobs) <= L.HIST_MAX_JOBS:
        raise BnnHipError(f"param_hist: 1 to {L.HIST_MAX_JOBS} jobs per call, got {len(jobs)}")
    a = L.ParamHistArgs()
    a.struct_bytes = C.sizeof(L.ParamHistArgs)
    a.n_jobs, a.n_edges = len(jobs), int(e.size)
    keep = [e]
    for i, job in enumerate(jobs):
        kind = int(job["kind"])
        if kind not in (L.HIST_VALUE, L.HIST_SIGMA, L.HIST_SNR_DB, L.HIST_SAMPLE):
            raise BnnHipError(f"param_hist: unknown kind {kind}")
        src0 = _hist_f32(job["src0"], "src0")
        j = a.jobs[i]
        j.kind, j.n, j.src0 = kind, src0.numel(), src0.data_ptr()
        keep.append(src0)
        if kind in (L.HIST_SNR_DB, L.HIST_SAMPLE):
            src1 = _hist_f32(job.get("src1"), "src1")
            if src1.numel() != src0.numel():
                raise BnnHipError("param_hist: src0 and src1 must have the same number of elements")
            j.src1 = src1.data_ptr()
            keep.append(src1)
        if kind == L.HIST_SAMPLE:
            j.rows, j.cols = (1, src0.numel()) if src0.dim() < 2 else (src0.numel() // src0.shape[-1], src0.shape[-1])
            j.seed = int(job.get("seed", 0)) & 0xFFFFFFFFFFFFFFFF
            j.tensor_id, j.sample = int(job.get("tensor_id", 0)) & 0xFFFFFFFF, int(job.get("sample", 0)) & 0xFFFFFFFF
        out = job.get("values_out")
        if out is not None:
            if _hist_f32(out, "values_out").numel() != src0.numel():
                raise BnnHipError("param_hist: values_out must have src0's number of elements")
            j.values_out = out.data_ptr()
            keep.append(out)
    require_device(*keep[1:])
    dev = keep[1].device
    words = L.hist_record_bytes(e.size) // 8
    if records is None:
        records = torch.zeros((len(jobs), words), dtype=torch.int64, device=dev)
    if records.dtype != torch.int64 or not records.is_contiguous() or tuple(records.shape) != (len(jobs), words):
        raise BnnHipError(f"param_hist: records must be a contiguous int64 [{len(jobs)}, {words}] tensor")
    require_device(records)
    for i in range(len(jobs)):
        a.jobs[i].record = records.data_ptr() + 8 * words * i
    edges_device = torch.from_numpy(e).to(dev)
    a.edges, a.edges_host = edges_device.data_ptr(), e.ctypes.data
    need = int(L.load().bnn_param_hist_workspace_bytes(C.byref(a)))
    if need == 0:
        raise BnnHipError("param_hist: the job list is outside the library's limits")
    if workspace is None:
        workspace = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
    require_device(workspace)
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    keep += [records, edges_device, workspace]
    a._keep, a.records, a.workspace_t, a.edges_device, a.edges_np = keep, records, workspace, edges_device, e
    return a


def param_hist(a: L.ParamHistArgs):
    """bnn_param_hist: clear, bin and fold into a.records on the current stream; nothing is read back."""
    L.check(L.load().bnn_param_hist(C.byref(a), _stream()), "bnn_param_hist")


# ---------------------------------------------------------------------------------------------------------------- F12 held-out scores
@dataclass(frozen=True)
class ClassificationScore:
    """Scores.read() of a classification record: per-row means, and the top-label reliability bins ((i / M, (i + 1) / M])
    of the MC-mean prediction.  ece = sum_b |sum conf_b - correct_b| / n, mce = the largest |confidence - accuracy| over the
    non-empty bins; bin_accuracy / bin_confidence are NaN for an empty bin."""
    n: int
    accuracy: float
    lpd: float
    nll: float
    brier: float
    ece: float
    mce: float
    bin_count: "object"
    bin_accuracy: "object"
    bin_confidence: "object"


@dataclass(frozen=True)
class RegressionScore:
    """Scores.read() of a regression record: n counts output elements (rows * outputs); lpd / nll are per element; `pit` are
    the counts of the probability integral transform's M equal bins over [0, 1]."""
    n: int
    rows: int
    rmse: float
    mae: float
    lpd: float
    nll: float
    pit: "object"

    def coverage(self, level: float) -> float:
        """The share of elements whose PIT lies in [1/2 - level/2, 1/2 + level/2): the empirical coverage of the central
        `level` predictive interval, read off the histogram.  Raises unless M is even and level * M / 2 is an integer in
        [1, M / 2] -- the histogram cannot answer otherwise."""
        M = len(self.pit)
        half = float(level) * M / 2.0
        k = int(round(half))
        if M < 2 or M % 2 or abs(half - k) > 1e-9 or not 1 <= k <= M // 2:
            raise BnnHipError(f"coverage({level}): {M} PIT bins cannot answer (M must be even and level * M / 2 an integer in [1, M / 2])")
        return float(self.pit[M // 2 - k:M // 2 + k].sum()) / self.n if self.n else float("nan")


def parse_score_record(words, mode: str, bins: int):
    """A host copy of a bnn_mc_score record (int64 [8 + 3 * bins]) as a ClassificationScore / RegressionScore."""
    import numpy as np
    w = np.ascontiguousarray(np.asarray(words, dtype=np.int64).reshape(-1))
    M = int(bins)
    if w.size != 8 + 3 * M:
        raise BnnHipError(f"score record: {8 + 3 * M} words for {M} bins, got {w.size}")
    f = w.view(np.float64)
    b = w[8:].reshape(M, 3)
    count = b[:, 0].copy()
    n = int(w[0])
    with np.errstate(invalid="ignore", divide="ignore"):
        if mode == "classification":
            ok, conf = b[:, 1].astype(np.float64), b[:, 2].copy().view(np.float64)
            gap = np.abs(conf - ok)
            live = count > 0
            mce = float((gap[live] / count[live]).max()) if live.any() else 0.0
            d = float(n) if n else float("nan")
            return ClassificationScore(n=n, accuracy=int(w[1]) / d, lpd=float(f[2]) / d, nll=float(f[3]) / d,
                                       brier=float(f[4]) / d, ece=float(gap.sum()) / d, mce=mce, bin_count=count,
                                       bin_accuracy=np.where(live, ok / count, np.nan),
                                       bin_confidence=np.where(live, conf / count, np.nan))
        if mode == "regression":
            ne = int(w[1])
            d = float(ne) if ne else float("nan")
            return RegressionScore(n=ne, rows=n, rmse=math.sqrt(float(f[4]) / d) if ne else float("nan"), mae=float(f[5]) / d,
                                   lpd=float(f[2]) / d, nll=float(f[3]) / d, pit=count)
    raise Exception("Training mode must be either 'regression' or 'classification'")


class Scores:
    """The device record of bnn_mc_score (include/bnn_hip.h F12) for one mode and bin count.  `accumulate(logits, targets)`
    adds a launch's rows to it and `reset()` zeroes it: both are capturable and read nothing.  `read()` is one
    device-to-host copy and returns a ClassificationScore / RegressionScore of plain Python floats and numpy arrays.
    With rows=True, `.row_lpd` / `.row_nll` hold the last launch's per-row values ([G, B] fp32; padding rows unwritten)."""

    def __init__(self, mode: str, bins: int = 10, device=None, record: Optional[torch.Tensor] = None):
        if mode not in ("classification", "regression"):
            raise Exception("Training mode must be either 'regression' or 'classification'")
        self.mode, self.bins = mode, int(bins)
        if not 0 <= self.bins <= L.SCORE_MAX_BINS:
            raise BnnHipError(f"Scores: bins must lie in [0, {L.SCORE_MAX_BINS}] (BNN_SCORE_MAX_BINS)")
        words = L.score_record_bytes(self.bins) // 8
        if record is None:
            if device is None:
                raise BnnHipError("Scores: a device (or a record tensor) is needed")
            record = torch.zeros(words, dtype=torch.int64, device=device)
        if record.dtype != torch.int64 or not record.is_contiguous() or record.numel() != words:
            raise BnnHipError(f"Scores: the record must be a contiguous int64 tensor of {words} words")
        self.record = record
        self.row_lpd = self.row_nll = None
        self._ws = {}

    def reset(self):
        self.record.zero_()
        return self

    def accumulate(self, logits: torch.Tensor, targets: torch.Tensor, *, groups: Optional[int] = None, sigma: float = 1.0,
                   n_valid: Optional[int] = None, rows: bool = False, overwrite: bool = False):
        """One bnn_mc_score call on the current stream.  logits: float32 [G, S, B, C], or [G * S, B, C] with `groups` (the
        stacked evaluation's output; groups = 1 by default); targets: int64 [G, B] labels or float32 [G, B, C]."""
        lib = L.load()
        require_device(logits, targets, self.record)
        lg = _f32c(logits, "logits")
        if lg.dim() == 4 and groups is None:
            G, S, B, Cc = lg.shape
        elif lg.dim() == 3 and lg.shape[0] % int(groups or 1) == 0:
            G = int(groups or 1)
            S, B, Cc = lg.shape[0] // G, lg.shape[1], lg.shape[2]
        else:
            raise BnnHipError("mc_score: logits must be [groups, samples, batch, outputs] or [groups * samples, batch, outputs]")
        cls = self.mode == "classification"
        want, dt = (G * B, torch.int64) if cls else (G * B * Cc, torch.float32)
        if targets.dtype != dt or targets.numel() != want:
            raise BnnHipError(f"mc_score: targets must be {dt} with {want} entries, got {targets.dtype} {tuple(targets.shape)}")
        tg = targets if targets.is_contiguous() else targets.contiguous()
        nv = G * B if n_valid is None else int(n_valid)
        if not 1 <= nv <= G * B:
            raise BnnHipError(f"mc_score: n_valid must lie in [1, {G * B}], got {nv}")
        if not cls and not float(sigma) > 0.0:
            raise BnnHipError("mc_score: sigma must be > 0")
        need = int(lib.bnn_mc_score_workspace_bytes(G, B, Cc))
        if need == 0:
            raise BnnHipError("mc_score: the shape is outside the library's limits")
        ws = self._ws.get(need)
        if ws is None:
            ws = self._ws[need] = torch.empty(need // 8 + 1, dtype=torch.int64, device=lg.device)
        a = L.McScoreArgs()
        a.struct_bytes = C.sizeof(L.McScoreArgs)
        a.mode = L.NLL_CLASSIFICATION if cls else L.NLL_REGRESSION
        a.groups, a.n_samples, a.batch, a.classes = G, S, B, Cc
        a.logits, a.targets, a.n_valid = lg.data_ptr(), tg.data_ptr(), nv
        a.sigma, a.n_bins, a.accumulate = float(sigma), self.bins, 0 if overwrite else 1
        if rows:
            if self.row_lpd is None or tuple(self.row_lpd.shape) != (G, B):
                self.row_lpd = torch.empty((G, B), dtype=torch.float32, device=lg.device)
                self.row_nll = torch.empty((G, B), dtype=torch.float32, device=lg.device)
            a.row_lpd, a.row_nll = self.row_lpd.data_ptr(), self.row_nll.data_ptr()
        a.record = self.record.data_ptr()
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 8
        a._keep = (lg, tg, ws, self.record, self.row_lpd, self.row_nll)
        L.check(lib.bnn_mc_score(C.byref(a), _stream()), "bnn_mc_score")
        return self

    def read(self):
        """One device-to-host copy of the record."""
        return parse_score_record(self.record.cpu().numpy(), self.mode, self.bins)


def mc_score(logits: torch.Tensor, targets: torch.Tensor, mode: str, *, sigma: float = 1.0, bins: int = 10,
             n_valid: Optional[int] = None, record: Optional[Scores] = None, rows: bool = False, groups: Optional[int] = None) -> Scores:
    """F12: bnn_mc_score over the MC outputs `logits` ([G, S, B, C], or [S, B, C] for one minibatch) and their targets.
    Without `record` a fresh Scores holds this call alone; with one (of the same mode) the call's rows are added to it.
    Rows with flat index g * B + b >= n_valid are padding: never loaded, never counted.  Nothing is read back before
    `.read()`."""
    if record is None:
        require_device(logits)
        return Scores(mode, bins, logits.device).accumulate(logits, targets, groups=groups, sigma=sigma, n_valid=n_valid,
                                                             rows=rows, overwrite=True)
    if record.mode != mode:
        raise BnnHipError(f"mc_score: the record holds {record.mode} scores, not {mode}")
    return record.accumulate(logits, targets, groups=groups, sigma=sigma, n_valid=n_valid, rows=rows)


# ---------------------------------------------------------------------------------------------------------------- F13 compressed network
def sparse_count(code: torch.Tensor, level: int, row_ptr: torch.Tensor, *, out_features: int, in_features: int):
    """bnn_sparse_count: row_ptr (int32 [out + 1]) = the exclusive scan of the per-row survivor counts (code > level) of the
    canonical [>= out, ld] uint8 code image; row_ptr[out] is nnz."""
    require_device(code, row_ptr)
    if code.dtype != torch.uint8 or code.dim() != 2 or not code.is_contiguous() or code.shape[0] < out_features:
        raise BnnHipError("sparse_count: code must be a contiguous uint8 [>= out_features, ld] image")
    if row_ptr.dtype != torch.int32 or not row_ptr.is_contiguous() or row_ptr.numel() != out_features + 1:
        raise BnnHipError("sparse_count: row_ptr must be int32 [out_features + 1]")
    a = L.SparseCountArgs()
    a.struct_bytes = C.sizeof(L.SparseCountArgs)
    a.out_features, a.in_features, a.ld, a.level = int(out_features), int(in_features), code.shape[1], int(level)
    a.code, a.row_ptr = code.data_ptr(), row_ptr.data_ptr()
    L.check(L.load().bnn_sparse_count(C.byref(a), _stream()), "bnn_sparse_count")
    return row_ptr


def sparse_fill(code: torch.Tensor, level: int, row_ptr: torch.Tensor, mu: torch.Tensor, rho: torch.Tensor, col: torch.Tensor,
                mu_val: torch.Tensor, rho_val: torch.Tensor, *, out_features: int, in_features: int, transposed: bool):
    """bnn_sparse_fill: the survivors' columns (uint16, viewed as int16 storage) and their fp32 mu / rho, ascending within
    a row, at the places row_ptr (from sparse_count, same code and level) gives them."""
    require_device(code, row_ptr, mu, rho, col, mu_val, rho_val)
    mu, rho = _f32c(mu, "mu"), _f32c(rho, "rho")
    if mu.numel() != out_features * in_features or rho.numel() != mu.numel():
        raise BnnHipError("sparse_fill: mu and rho must hold out_features * in_features elements")
    if code.dtype != torch.uint8 or code.dim() != 2 or not code.is_contiguous() or code.shape[0] < out_features:
        raise BnnHipError("sparse_fill: code must be a contiguous uint8 [>= out_features, ld] image")
    if col.dtype != torch.int16 or mu_val.dtype != torch.float32 or rho_val.dtype != torch.float32 or \
            not (col.numel() == mu_val.numel() == rho_val.numel()) or row_ptr.dtype != torch.int32 or row_ptr.numel() != out_features + 1:
        raise BnnHipError("sparse_fill: col int16 (uint16 bits), mu_val / rho_val float32, all [nnz]; row_ptr int32 [out + 1]")
    a = L.SparseFillArgs()
    a.struct_bytes = C.sizeof(L.SparseFillArgs)
    a.out_features, a.in_features, a.ld, a.level = int(out_features), int(in_features), code.shape[1], int(level)
    a.transposed = int(bool(transposed))
    a.code, a.row_ptr, a.mu, a.rho = code.data_ptr(), row_ptr.data_ptr(), mu.data_ptr(), rho.data_ptr()
    a.col, a.mu_val, a.rho_val = col.data_ptr(), mu_val.data_ptr(), rho_val.data_ptr()
    L.check(L.load().bnn_sparse_fill(C.byref(a), _stream()), "bnn_sparse_fill")


def sparse_fwd_args(*, row_ptr: torch.Tensor, col: torch.Tensor, mu_val: torch.Tensor, sigma_val: Optional[torch.Tensor],
                    b_mu: torch.Tensor, b_sigma: Optional[torch.Tensor], x: torch.Tensor, y: torch.Tensor, n_samples: int,
                    rows: int, in_features: int, out_features: int, eps_mode: int, relu: bool, x_per_sample: int = 0,
                    x_feature_major: bool = False, y_feature_major: bool = False, layer_id: int = 0, seed: int = 0,
                    sample_offset: int = 0, sample_counter: Optional[torch.Tensor] = None, sample_group: int = 0,
                    sample_group_stride: int = 0, eps: Optional[torch.Tensor] = None, eps_b: Optional[torch.Tensor] = None,
                    eps_dump: Optional[torch.Tensor] = None, eps_b_dump: Optional[torch.Tensor] = None,
                    x_scratch: Optional[torch.Tensor] = None) -> L.SparseFwdArgs:
    """The argument block of bnn_sparse_fwd for one layer (include/bnn_hip.h F13).  x [x_rows, rows, in] or, feature-major,
    [x_rows, in, rows]; y [S, rows, out] or [S, out, rows]; eps / eps_dump [S, nnz], eps_b / eps_b_dump [S, out]."""
    tensors = (row_ptr, col, mu_val, sigma_val, b_mu, b_sigma, x, y, sample_counter, eps, eps_b, eps_dump, eps_b_dump, x_scratch)
    require_device(*tensors)
    if any(t is not None and not t.is_contiguous() for t in tensors):
        raise BnnHipError("sparse_fwd: contiguous tensors")
    if row_ptr.dtype != torch.int32 or row_ptr.numel() != out_features + 1 or col.dtype != torch.int16:
        raise BnnHipError("sparse_fwd: row_ptr int32 [out + 1], col int16 (uint16 bits)")
    for name, t in (("mu_val", mu_val), ("sigma_val", sigma_val), ("b_mu", b_mu), ("b_sigma", b_sigma), ("x", x), ("y", y),
                    ("eps", eps), ("eps_b", eps_b), ("eps_dump", eps_dump), ("eps_b_dump", eps_b_dump), ("x_scratch", x_scratch)):
        if t is not None and t.dtype != torch.float32:
            raise BnnHipError(f"sparse_fwd: {name} must be float32")
    x_rows = 1 if x_per_sample == 0 else -(-int(n_samples) // int(x_per_sample))
    if x.numel() != x_rows * rows * in_features or y.numel() != n_samples * rows * out_features or b_mu.numel() != out_features:
        raise BnnHipError("sparse_fwd: x must hold x_rows * rows * in, y n_samples * rows * out and b_mu out elements")
    if x_scratch is not None and x_scratch.numel() < x.numel():
        raise BnnHipError("sparse_fwd: x_scratch must hold as many elements as x")
    if sample_counter is not None and sample_counter.dtype not in (torch.int32, torch.uint32):
        raise BnnHipError("sparse_fwd: sample_counter must be a 32-bit device word")
    a = L.SparseFwdArgs()
    a.struct_bytes = C.sizeof(L.SparseFwdArgs)
    a.n_samples, a.rows, a.in_features, a.out_features = int(n_samples), int(rows), int(in_features), int(out_features)
    a.eps_mode, a.relu, a.x_per_sample = int(eps_mode), int(bool(relu)), int(x_per_sample)
    a.x_feature_major, a.y_feature_major = int(bool(x_feature_major)), int(bool(y_feature_major))
    a.layer_id, a.sample_offset, a.seed = int(layer_id), int(sample_offset) & 0xFFFFFFFF, int(seed) & 0xFFFFFFFFFFFFFFFF
    a.sample_group, a.sample_group_stride = int(sample_group), int(sample_group_stride)
    a.sample_counter, a.row_ptr, a.col, a.mu_val, a.sigma_val = _ptr(sample_counter), row_ptr.data_ptr(), col.data_ptr(), mu_val.data_ptr(), _ptr(sigma_val)
    a.b_mu, a.b_sigma, a.x, a.y = b_mu.data_ptr(), _ptr(b_sigma), x.data_ptr(), y.data_ptr()
    a.eps, a.eps_b, a.eps_dump, a.eps_b_dump, a.x_scratch = _ptr(eps), _ptr(eps_b), _ptr(eps_dump), _ptr(eps_b_dump), _ptr(x_scratch)
    a._keep = tensors                 # (the structure owns what its pointers refer to)
    return a


def sparse_fwd(a: L.SparseFwdArgs):
    L.check(L.load().bnn_sparse_fwd(C.byref(a), _stream()), "bnn_sparse_fwd")


# ---------------------------------------------------------------------------------------------------------------- F14 sparse training
def _u8c(t: torch.Tensor, name: str, numel: int) -> torch.Tensor:
    if t.dtype != torch.uint8 or not t.is_contiguous() or t.numel() != numel:
        raise BnnHipError(f"{name} must be a contiguous uint8 tensor of {numel} elements")
    return t


def sparse_elbo_terms_workspace(layers: Sequence[dict], n_samples: int, device) -> torch.Tensor:
    """The partials of bnn_sparse_elbo_terms for `layers` (dicts with nnz and out_features) and n_samples."""
    n = len(layers)
    nnz = (C.c_int32 * n)(*[int(l["nnz"]) for l in layers])
    outs = (C.c_int32 * n)(*[int(l["out_features"]) for l in layers])
    nb = L.load().bnn_sparse_elbo_terms_workspace_bytes(n, int(n_samples), nnz, outs)
    if nb == 0:
        raise BnnHipError("sparse_elbo_terms: 1 to 8 layers, 1 to 65535 samples")
    return torch.empty(nb // 4, dtype=torch.float32, device=device)


def sparse_elbo_terms_args(layers: Sequence[dict], *, n_samples: int, prior: PriorSpec, log_prior: torch.Tensor, log_q: torch.Tensor,
                           workspace: torch.Tensor, seed: int = 0, sample_offset: int = 0,
                           sample_counter: Optional[torch.Tensor] = None) -> L.SparseElboArgs:
    """The argument block of bnn_sparse_elbo_terms (include/bnn_hip.h F14).  A layer: dict(row_ptr, col, mu_val, sigma_val,
    b_mu, b_sigma, b_keep (uint8 [out]), in_features, out_features, nnz, layer_id)."""
    if not 1 <= len(layers) <= L.SPARSE_MAX_LAYERS:
        raise BnnHipError(f"sparse_elbo_terms: 1 to {L.SPARSE_MAX_LAYERS} layers")
    a = L.SparseElboArgs()
    a.struct_bytes = C.sizeof(L.SparseElboArgs)
    a.n_layers, a.n_samples = len(layers), int(n_samples)
    a.sample_offset, a.seed = int(sample_offset) & 0xFFFFFFFF, int(seed) & 0xFFFFFFFFFFFFFFFF
    a.prior = prior.c()
    keep = [log_prior, log_q, workspace, sample_counter]
    require_device(*keep)
    for i, l in enumerate(layers):
        ts = [l[k] for k in ("row_ptr", "col", "mu_val", "sigma_val", "b_mu", "b_sigma", "b_keep")]
        require_device(*ts)
        if any(not t.is_contiguous() for t in ts):
            raise BnnHipError("sparse_elbo_terms: contiguous tensors")
        out = int(l["out_features"])
        if l["row_ptr"].dtype != torch.int32 or l["row_ptr"].numel() != out + 1 or l["col"].dtype != torch.int16:
            raise BnnHipError("sparse_elbo_terms: row_ptr int32 [out + 1], col int16 (uint16 bits)")
        for k in ("mu_val", "sigma_val", "b_mu", "b_sigma"):
            if l[k].dtype != torch.float32:
                raise BnnHipError(f"sparse_elbo_terms: {k} must be float32")
        if l["mu_val"].numel() < int(l["nnz"]) or l["sigma_val"].numel() < int(l["nnz"]) or l["b_mu"].numel() != out:
            raise BnnHipError("sparse_elbo_terms: mu_val / sigma_val must hold nnz elements, the bias vectors out")
        _u8c(l["b_keep"], "sparse_elbo_terms: b_keep", out)
        y = a.layer[i]
        y.in_features, y.out_features, y.nnz, y.layer_id = int(l["in_features"]), out, int(l["nnz"]), int(l["layer_id"])
        y.row_ptr, y.col, y.mu_val, y.sigma_val = (l[k].data_ptr() for k in ("row_ptr", "col", "mu_val", "sigma_val"))
        y.b_mu, y.b_sigma, y.b_keep = (l[k].data_ptr() for k in ("b_mu", "b_sigma", "b_keep"))
        keep += ts
    if log_prior.dtype != torch.float32 or log_q.dtype != torch.float32 or log_prior.numel() != n_samples or log_q.numel() != n_samples:
        raise BnnHipError("sparse_elbo_terms: log_prior and log_q must be float32 [n_samples]")
    a.sample_counter, a.log_prior, a.log_q = _ptr(sample_counter), log_prior.data_ptr(), log_q.data_ptr()
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    a._keep = keep
    return a


def sparse_elbo_terms(a: L.SparseElboArgs):
    L.check(L.load().bnn_sparse_elbo_terms(C.byref(a), _stream()), "bnn_sparse_elbo_terms")


def sparse_bwd_workspace(n_samples: int, rows: int, out_features: int, device) -> torch.Tensor:
    nb = L.load().bnn_sparse_bwd_workspace_bytes(int(n_samples), int(rows), int(out_features))
    if nb == 0:
        raise BnnHipError("sparse_bwd: positive dimensions, at most 65535 samples")
    return torch.empty(nb // 4, dtype=torch.float32, device=device)


def sparse_bwd_args(*, row_ptr: torch.Tensor, col: torch.Tensor, mu_val: torch.Tensor, rho_val: torch.Tensor, b_mu: torch.Tensor,
                    b_rho: torch.Tensor, b_keep: torch.Tensor, x: torch.Tensor, gy: torch.Tensor, y: Optional[torch.Tensor],
                    g_mu_val: torch.Tensor, g_rho_val: torch.Tensor, g_b_mu: torch.Tensor, g_b_rho: torch.Tensor,
                    workspace: Optional[torch.Tensor], n_samples: int, rows: int, in_features: int, out_features: int, nnz: int,
                    prior: PriorSpec, relu: bool, gy_row_major: bool, x_per_sample: int = 0, gx_relu_mask: bool = False,
                    layer_id: int = 0, seed: int = 0, sample_offset: int = 0, sample_counter: Optional[torch.Tensor] = None,
                    g_log_prior: Optional[torch.Tensor] = None, g_log_q: Optional[torch.Tensor] = None,
                    g_x: Optional[torch.Tensor] = None, col_ptr: Optional[torch.Tensor] = None, row: Optional[torch.Tensor] = None,
                    perm: Optional[torch.Tensor] = None) -> L.SparseBwdArgs:
    """The argument block of bnn_sparse_bwd for one layer (include/bnn_hip.h F14).  x [x_rows, in, rows] and y [S, out, rows]
    feature-major; gy [S, rows, out] (gy_row_major) or [S, out, rows]; g_x [S, in, rows] with the CSC view (col_ptr, row, perm)."""
    f32 = dict(mu_val=mu_val, rho_val=rho_val, b_mu=b_mu, b_rho=b_rho, x=x, gy=gy, y=y, g_mu_val=g_mu_val, g_rho_val=g_rho_val,
               g_b_mu=g_b_mu, g_b_rho=g_b_rho, workspace=workspace, g_log_prior=g_log_prior, g_log_q=g_log_q, g_x=g_x)
    tensors = list(f32.values()) + [row_ptr, col, b_keep, sample_counter, col_ptr, row, perm]
    require_device(*tensors)
    if any(t is not None and not t.is_contiguous() for t in tensors):
        raise BnnHipError("sparse_bwd: contiguous tensors")
    for name, t in f32.items():
        if t is not None and t.dtype != torch.float32:
            raise BnnHipError(f"sparse_bwd: {name} must be float32")
    S, nnz = int(n_samples), int(nnz)
    if row_ptr.dtype != torch.int32 or row_ptr.numel() != out_features + 1 or col.dtype != torch.int16:
        raise BnnHipError("sparse_bwd: row_ptr int32 [out + 1], col int16 (uint16 bits)")
    _u8c(b_keep, "sparse_bwd: b_keep", out_features)
    x_rows = 1 if x_per_sample == 0 else -(-S // int(x_per_sample))
    if x.numel() != x_rows * rows * in_features or gy.numel() != S * rows * out_features or \
            (y is not None and y.numel() != gy.numel()) or (g_x is not None and g_x.numel() != S * rows * in_features):
        raise BnnHipError("sparse_bwd: x must hold x_rows * rows * in, gy and y n_samples * rows * out, g_x n_samples * rows * in elements")
    if min(t.numel() for t in (col, mu_val, rho_val, g_mu_val, g_rho_val)) < nnz or \
            any(t.numel() != out_features for t in (b_mu, b_rho, g_b_mu, g_b_rho)):
        raise BnnHipError("sparse_bwd: the value arrays must hold nnz elements, the bias vectors out_features")
    if any(t is not None and t.numel() != S for t in (g_log_prior, g_log_q)):
        raise BnnHipError("sparse_bwd: g_log_prior / g_log_q must hold n_samples elements")
    if g_x is not None:
        if col_ptr is None or row is None or perm is None or col_ptr.dtype != torch.int32 or col_ptr.numel() != in_features + 1 or \
                row.dtype != torch.int16 or perm.dtype != torch.int32 or row.numel() < nnz or perm.numel() < nnz:
            raise BnnHipError("sparse_bwd: g_x needs the CSC view: col_ptr int32 [in + 1], row int16 (uint16 bits) [nnz], perm int32 [nnz]")
    a = L.SparseBwdArgs()
    a.struct_bytes = C.sizeof(L.SparseBwdArgs)
    a.n_samples, a.rows, a.in_features, a.out_features, a.nnz = S, int(rows), int(in_features), int(out_features), nnz
    a.relu, a.gy_row_major, a.x_per_sample, a.gx_relu_mask = int(bool(relu)), int(bool(gy_row_major)), int(x_per_sample), int(bool(gx_relu_mask))
    a.layer_id, a.sample_offset, a.seed = int(layer_id), int(sample_offset) & 0xFFFFFFFF, int(seed) & 0xFFFFFFFFFFFFFFFF
    a.prior = prior.c()
    a.sample_counter, a.row_ptr, a.col, a.mu_val, a.rho_val = _ptr(sample_counter), row_ptr.data_ptr(), col.data_ptr(), mu_val.data_ptr(), rho_val.data_ptr()
    a.col_ptr, a.row, a.perm = _ptr(col_ptr), _ptr(row), _ptr(perm)
    a.b_mu, a.b_rho, a.b_keep, a.x, a.y, a.gy = b_mu.data_ptr(), b_rho.data_ptr(), b_keep.data_ptr(), x.data_ptr(), _ptr(y), gy.data_ptr()
    a.g_log_prior, a.g_log_q = _ptr(g_log_prior), _ptr(g_log_q)
    a.g_mu_val, a.g_rho_val, a.g_b_mu, a.g_b_rho, a.g_x = g_mu_val.data_ptr(), g_rho_val.data_ptr(), g_b_mu.data_ptr(), g_b_rho.data_ptr(), _ptr(g_x)
    a.workspace = _ptr(workspace)                            # read only when the gz launch runs (relu or gy_row_major)
    a.workspace_bytes = workspace.numel() * workspace.element_size() if workspace is not None else 0
    a._keep = tensors
    return a


def sparse_bwd(a: L.SparseBwdArgs):
    L.check(L.load().bnn_sparse_bwd(C.byref(a), _stream()), "bnn_sparse_bwd")


def sparse_sigma_args(segments: Sequence[tuple]) -> L.SparseSigmaArgs:
    """The argument block of bnn_sparse_sigma_refresh: segments of (rho, sigma, keep uint8 or None, n): sigma[:n] =
    keep ? softplus(rho[:n]) : 0."""
    if not 1 <= len(segments) <= L.SPARSE_MAX_SEGMENTS:
        raise BnnHipError(f"sparse_sigma_refresh: 1 to {L.SPARSE_MAX_SEGMENTS} segments")
    a = L.SparseSigmaArgs()
    a.struct_bytes = C.sizeof(L.SparseSigmaArgs)
    a.n_segments = len(segments)
    keep_alive = []
    for i, (rho, sigma, keep, n) in enumerate(segments):
        require_device(rho, sigma, keep)
        n = int(n)
        if rho.dtype != torch.float32 or sigma.dtype != torch.float32 or not rho.is_contiguous() or not sigma.is_contiguous() or \
                rho.numel() < n or sigma.numel() < n:
            raise BnnHipError("sparse_sigma_refresh: rho and sigma must be contiguous float32 of at least n elements")
        if keep is not None:
            _u8c(keep, "sparse_sigma_refresh: keep", n)
        a.rho[i], a.sigma[i], a.keep[i], a.n[i] = rho.data_ptr(), sigma.data_ptr(), _ptr(keep), n
        keep_alive += [rho, sigma, keep]
    a._keep = keep_alive
    return a


def sparse_sigma_refresh(a: L.SparseSigmaArgs):
    L.check(L.load().bnn_sparse_sigma_refresh(C.byref(a), _stream()), "bnn_sparse_sigma_refresh")


# ---------------------------------------------------------------------------------------------------------------- F15 BatchBALD
def batchbald_configs(n_classes: int, n_chosen: int, max_configs: int) -> int:
    """bnn_batchbald_configs on the host: rows of Phat when n_chosen rows are in the batch -- C^n while that does not
    exceed max_configs, else max_configs."""
    m = 1
    for _ in range(int(n_chosen)):
        m *= int(n_classes)
        if m > int(max_configs):
            return int(max_configs)
    return m


def _batchbald_dims(what, S, N, Cc):
    if not (2 <= Cc <= L.BATCHBALD_MAX_CLASSES and 1 <= S <= L.BATCHBALD_MAX_SAMPLES and 1 <= N <= L.EPOCH_MAX_ROWS):
        raise BnnHipError(f"{what}: classes must lie in [2, {L.BATCHBALD_MAX_CLASSES}], samples in [1, {L.BATCHBALD_MAX_SAMPLES}], "
                          f"rows in [1, {L.EPOCH_MAX_ROWS}]; got {Cc}, {S}, {N}")


def batchbald_probs(logits: torch.Tensor, probs: torch.Tensor, cond: torch.Tensor, marg: torch.Tensor, row0: int):
    """bnn_batchbald_probs: logits float32 [S, B, C] of pool rows row0 .. row0 + B - 1 into probs float32 [S, N, C] and the
    float64 [N] entropies cond (expected) and marg (of the mean)."""
    if logits.dim() != 3 or probs.dim() != 3:
        raise BnnHipError("batchbald_probs: logits [S, B, C] and probs [S, N, C]")
    S, B, Cc = logits.shape
    N = probs.shape[1]
    _batchbald_dims("batchbald_probs", S, N, Cc)
    if probs.shape[0] != S or probs.shape[2] != Cc or not 0 <= int(row0) <= N - B:
        raise BnnHipError("batchbald_probs: probs must be [S, N, C] with row0 + B <= N")
    keep = [_typed(logits, torch.float32, "logits"), _typed(probs, torch.float32, "probs"), _typed(cond, torch.float64, "cond", N),
            _typed(marg, torch.float64, "marg", N)]
    a = L.BatchBaldProbsArgs()
    a.struct_bytes = C.sizeof(L.BatchBaldProbsArgs)
    a.n_samples, a.n_rows, a.n_classes, a.row0, a.chunk_rows = S, N, Cc, int(row0), B
    a.logits, a.probs, a.cond, a.marg = (t.data_ptr() for t in keep)
    L.check(L.load().bnn_batchbald_probs(C.byref(a), _stream()), "bnn_batchbald_probs")


def batchbald_joint_workspace(n_rows: int, n_classes: int, n_configs: int, device) -> torch.Tensor:
    """bnn_batchbald_joint's workspace for up to n_configs rows of Phat (any contents; 8-byte aligned)."""
    nbytes = L.load().bnn_batchbald_joint_workspace_bytes(int(n_rows), int(n_classes), int(n_configs))
    return torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=device)


def batchbald_joint_args(*, probs, phat, weight, offset, cond, base, scores, n_configs: int, scores64=None, joint64=None,
                         workspace=None) -> L.BatchBaldJointArgs:
    """The argument block of bnn_batchbald_joint (include/bnn_hip.h F15): probs float32 [S, N, C], phat float32 [>= M, S],
    weight / offset float64 [>= M], cond float64 [N], base one float64 device word, scores float32 [N], scores64 / joint64
    optional float64 [N]."""
    if probs.dim() != 3:
        raise BnnHipError("batchbald_joint: probs [S, N, C]")
    S, N, Cc = probs.shape
    M = int(n_configs)
    _batchbald_dims("batchbald_joint", S, N, Cc)
    if not 1 <= M <= L.BATCHBALD_MAX_CONFIGS:
        raise BnnHipError(f"batchbald_joint: n_configs must lie in [1, {L.BATCHBALD_MAX_CONFIGS}]")
    keep = [_typed(probs, torch.float32, "probs"), _typed(phat, torch.float32, "phat"), _typed(weight, torch.float64, "weight"),
            _typed(offset, torch.float64, "offset"), _typed(cond, torch.float64, "cond", N), _typed(base, torch.float64, "base", 1),
            _typed(scores, torch.float32, "scores", N)]
    if phat.numel() < M * S or weight.numel() < M or offset.numel() < M:
        raise BnnHipError("batchbald_joint: phat, weight and offset must hold n_configs rows")
    a = L.BatchBaldJointArgs()
    a.struct_bytes = C.sizeof(L.BatchBaldJointArgs)
    a.n_samples, a.n_rows, a.n_classes, a.n_configs = S, N, Cc, M
    a.probs, a.phat, a.weight, a.offset, a.cond, a.base, a.scores = (t.data_ptr() for t in keep)
    for name, t in (("scores64", scores64), ("joint64", joint64)):
        if t is not None:
            keep.append(_typed(t, torch.float64, name, N))
            setattr(a, name, t.data_ptr())
    if workspace is None:
        workspace = batchbald_joint_workspace(N, Cc, M, probs.device)
    require_device(workspace)
    keep.append(workspace)
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    a._keep = keep
    return a


def batchbald_joint(a: L.BatchBaldJointArgs):
    """bnn_batchbald_joint: scores[i] = H(chosen rows, row i) - cond[i] - base for every row of the pool."""
    L.check(L.load().bnn_batchbald_joint(C.byref(a), _stream()), "bnn_batchbald_joint")


def batchbald_state_args(*, probs, cond, labelled, n_labelled, phat_in, expo_in, phat_out, expo_out, weight, offset, base,
                         max_configs: int, n_chosen: int = 0, round: int = 0, seed: int = 0, scores64=None,
                         batch_scores=None, last: bool = False) -> L.BatchBaldStateArgs:
    """The argument block of bnn_batchbald_begin / bnn_batchbald_extend (include/bnn_hip.h F15).  The state tensors must
    hold bnn_batchbald_configs rows for the step they serve: phat float32 [M, S], expo int32 [M], weight / offset float64
    [M]; phat_in / expo_in and phat_out / expo_out are different tensors.  `last`: the extend of a batch's last row, which
    writes base and batch_scores only (the state tensors are not sized for it)."""
    if probs.dim() != 3:
        raise BnnHipError("batchbald_state: probs [S, N, C]")
    S, N, Cc = probs.shape
    _batchbald_dims("batchbald_state", S, N, Cc)
    mc, n = int(max_configs), int(n_chosen)
    if not 1 <= mc <= L.BATCHBALD_MAX_CONFIGS or not 0 <= n <= L.BATCHBALD_MAX_K:
        raise BnnHipError(f"batchbald_state: max_configs must lie in [1, {L.BATCHBALD_MAX_CONFIGS}], n_chosen in "
                          f"[0, {L.BATCHBALD_MAX_K}] (BNN_BATCHBALD_MAX_K)")
    m_out, m_in = batchbald_configs(Cc, n, mc), batchbald_configs(Cc, max(n - 1, 0), mc)
    if last:
        m_out = 0
    keep = [_typed(probs, torch.float32, "probs"), _typed(cond, torch.float64, "cond", N),
            _typed(labelled, torch.int32, "labelled", N), _typed(n_labelled, torch.int32, "n_labelled", 1),
            _typed(phat_in, torch.float32, "phat_in"), _typed(expo_in, torch.int32, "expo_in"),
            _typed(phat_out, torch.float32, "phat_out"), _typed(expo_out, torch.int32, "expo_out"),
            _typed(weight, torch.float64, "weight"), _typed(offset, torch.float64, "offset"), _typed(base, torch.float64, "base", 1)]
    if phat_in.numel() < m_in * S or expo_in.numel() < m_in or phat_out.numel() < m_out * S or expo_out.numel() < m_out or \
            weight.numel() < m_out or offset.numel() < m_out:
        raise BnnHipError(f"batchbald_state: the state tensors must hold {m_in} rows in and {m_out} rows out")
    if phat_in.data_ptr() == phat_out.data_ptr() or expo_in.data_ptr() == expo_out.data_ptr():
        raise BnnHipError("batchbald_state: the in and out state must be different tensors")
    a = L.BatchBaldStateArgs()
    a.struct_bytes = C.sizeof(L.BatchBaldStateArgs)
    a.n_samples, a.n_rows, a.n_classes, a.max_configs, a.n_chosen = S, N, Cc, mc, n
    a.round, a.seed, a.last = int(round) & 0xFFFFFFFF, int(seed) & 0xFFFFFFFFFFFFFFFF, int(bool(last))
    (a.probs, a.cond, a.labelled, a.n_labelled, a.phat_in, a.expo_in, a.phat_out, a.expo_out, a.weight, a.offset,
     a.base) = (t.data_ptr() for t in keep)
    if scores64 is not None:
        keep.append(_typed(scores64, torch.float64, "scores64", N))
        a.scores64 = scores64.data_ptr()
    if batch_scores is not None:
        if scores64 is None or batch_scores.numel() < n:
            raise BnnHipError("batchbald_state: batch_scores needs scores64 and n_chosen entries")
        keep.append(_typed(batch_scores, torch.float64, "batch_scores"))
        a.batch_scores = batch_scores.data_ptr()
    a._keep = keep
    return a


def batchbald_begin(a: L.BatchBaldStateArgs):
    """bnn_batchbald_begin: the empty batch into (phat_out, expo_out, weight, offset, base)."""
    L.check(L.load().bnn_batchbald_begin(C.byref(a), _stream()), "bnn_batchbald_begin")


def batchbald_extend(a: L.BatchBaldStateArgs):
    """bnn_batchbald_extend: the winner bnn_acquire_topk just appended folded into the state of the next step."""
    L.check(L.load().bnn_batchbald_extend(C.byref(a), _stream()), "bnn_batchbald_extend")


# ---------------------------------------------------------------------------------------------- F16: Flipout
def _flipout_math(math_mode: int) -> int:
    if math_mode == L.MATH_BF16X3:
        raise BnnHipError("Flipout has no split-bf16 (bf16x3) form: use bnn_hip.set_math('bf16') or set_math('f32')")
    return math_mode


def flipout_signs(seed: int, layer_id: int, kind: int, sample_offset: int, n_samples: int, rows: int, cols: int, device,
                  row_offset: int = 0) -> torch.Tensor:
    """The Flipout sign stream, materialised: int8[n_samples, rows, cols] of +1 / -1 (kind 0: input signs r, 1: output signs s)."""
    lib = L.load()
    if torch.device(device).type != "cuda":
        raise BnnHipError("bnn_hip.flipout_signs needs a ROCm device")
    out = torch.empty((n_samples, rows, cols), dtype=torch.int8, device=device)
    a = L.FlipoutSignsArgs(C.sizeof(L.FlipoutSignsArgs), n_samples, rows, cols, kind, layer_id, sample_offset & 0xFFFFFFFF,
                           row_offset & 0xFFFFFFFF, seed & 0xFFFFFFFFFFFFFFFF, out.data_ptr())
    L.check(lib.bnn_flipout_signs(C.byref(a), _stream()), "bnn_flipout_signs")
    return out


def flipout_prepare(w_mu, w_rho, b_mu, b_rho, *, n_samples: int, n_draws: int, prior: PriorSpec, math_mode: int, eps_mode: int,
                    eps_w=None, eps_b=None, seed: int = 0, layer_id: int = 0, sample_offset: int = 0, sample_counter=None,
                    want_stats: bool = False, want_eps: bool = False) -> dict:
    """Everything of a Flipout layer that depends on no activation (bnn_flipout_prepare): delta [D, out, in], b_draw [D, out],
    in bf16 math their bf16 copies and mu's, with want_stats log_prior[D] / log_q[D], with want_eps the epsilon used."""
    lib = L.load()
    require_device(w_mu, w_rho, b_mu, b_rho, eps_w, eps_b)
    math_mode = _flipout_math(math_mode)
    N, K = w_mu.shape
    D, dev = int(n_draws), w_mu.device
    w_mu, w_rho, b_mu, b_rho = (_f32c(t, n) for t, n in ((w_mu, "w_mu"), (w_rho, "w_rho"), (b_mu, "b_mu"), (b_rho, "b_rho")))
    if eps_mode == L.EPS_MEMORY:
        eps_w, eps_b = _f32c(eps_w, "eps_w"), _f32c(eps_b, "eps_b")
        if tuple(eps_w.shape) != (D, N, K) or tuple(eps_b.shape) != (D, N):
            raise BnnHipError(f"flipout_prepare: injected eps must be [{D}, {N}, {K}] and [{D}, {N}] (one per base draw)")
    bf16 = math_mode == L.MATH_BF16
    out = dict(delta=torch.empty((D, N, K), dtype=torch.float32, device=dev), b_draw=torch.empty((D, N), dtype=torch.float32, device=dev),
               delta_bf16=torch.empty((D, N, K), dtype=torch.bfloat16, device=dev) if bf16 else None,
               mu_bf16=torch.empty((N, K), dtype=torch.bfloat16, device=dev) if bf16 else None,
               log_prior=torch.empty(D, dtype=torch.float32, device=dev) if want_stats else None,
               log_q=torch.empty(D, dtype=torch.float32, device=dev) if want_stats else None,
               eps_w=torch.empty((D, N, K), dtype=torch.float32, device=dev) if want_eps else None,
               eps_b=torch.empty((D, N), dtype=torch.float32, device=dev) if want_eps else None)
    ws = None
    if want_stats:
        ws = torch.empty(max(1, lib.bnn_flipout_prepare_workspace_bytes(D, K, N) // 8), dtype=torch.float64, device=dev)
    a = L.FlipoutPrepareArgs()
    a.struct_bytes = C.sizeof(L.FlipoutPrepareArgs)
    a.n_samples, a.n_draws, a.in_features, a.out_features = int(n_samples), D, K, N
    a.eps_mode, a.math = eps_mode, math_mode
    a.layer_id, a.sample_offset = layer_id, sample_offset & 0xFFFFFFFF
    a.seed, a.sample_counter = seed & 0xFFFFFFFFFFFFFFFF, _ptr(sample_counter)
    a.w_mu, a.w_rho, a.b_mu, a.b_rho = w_mu.data_ptr(), w_rho.data_ptr(), b_mu.data_ptr(), b_rho.data_ptr()
    a.eps_w, a.eps_b = _ptr(eps_w), _ptr(eps_b)
    a.prior, a.want_stats = prior.c(), int(bool(want_stats))
    a.delta, a.b_draw, a.delta_bf16, a.mu_bf16 = out["delta"].data_ptr(), out["b_draw"].data_ptr(), _ptr(out["delta_bf16"]), _ptr(out["mu_bf16"])
    a.log_prior, a.log_q, a.eps_w_dump, a.eps_b_dump = _ptr(out["log_prior"]), _ptr(out["log_q"]), _ptr(out["eps_w"]), _ptr(out["eps_b"])
    a.workspace, a.workspace_bytes = _ptr(ws), 0 if ws is None else ws.numel() * 8
    L.check(lib.bnn_flipout_prepare(C.byref(a), _stream()), "bnn_flipout_prepare")
    out["_keep"] = (w_mu, w_rho, b_mu, b_rho, eps_w, eps_b, ws, sample_counter)
    return out


def flipout_fwd(x, prep: dict, w_mu, b_mu, *, n_samples: int, n_draws: int, math_mode: int, relu: bool, eps_mode: int,
                y_dtype: torch.dtype = torch.float32, seed: int = 0, layer_id: int = 0, sample_offset: int = 0, sample_counter=None,
                row_offset: int = 0) -> torch.Tensor:
    """The Flipout layer (bnn_flipout_fwd) over flipout_prepare's operands: x [batch, in] (one minibatch for every sample) or
    [S, batch, in] -> y [S, batch, out].  BNN_EPS_ZERO (prep may be None then, except in bf16 math): y = act(x mu^T + b_mu)."""
    lib = L.load()
    require_device(x, w_mu)
    math_mode = _flipout_math(math_mode)
    S, D = int(n_samples), int(n_draws)
    N, K = w_mu.shape
    if x.dim() not in (2, 3) or x.shape[-1] != K or (x.dim() == 3 and x.shape[0] != S):
        raise BnnHipError(f"flipout_fwd: x must be [batch, {K}] or [{S}, batch, {K}], got {tuple(x.shape)}")
    x = x if x.is_contiguous() else x.contiguous()
    B = x.shape[-2]
    bf16 = math_mode == L.MATH_BF16
    if not bf16 and x.dtype != torch.float32:
        raise BnnHipError("flipout_fwd: exact-fp32 math takes float32 activations")
    zero = eps_mode == L.EPS_ZERO
    y = torch.empty((S, B, N), dtype=y_dtype if bf16 else torch.float32, device=x.device)
    a = L.FlipoutFwdArgs()
    a.struct_bytes = C.sizeof(L.FlipoutFwdArgs)
    a.n_samples, a.n_draws, a.batch, a.in_features, a.out_features = S, D, B, K, N
    a.x_dtype, a.x_per_sample, a.math, a.eps_mode = _dt(x), int(x.dim() == 3), math_mode, eps_mode
    a.relu, a.y_dtype = int(bool(relu)), _dt(y)
    a.layer_id, a.sample_offset, a.row_offset = layer_id, sample_offset & 0xFFFFFFFF, row_offset & 0xFFFFFFFF
    a.seed, a.sample_counter, a.x = seed & 0xFFFFFFFFFFFFFFFF, _ptr(sample_counter), x.data_ptr()
    w_mu = _f32c(w_mu, "w_mu")
    b = _f32c(b_mu, "b_mu") if zero else prep["b_draw"]
    a.w_mu = w_mu.data_ptr()
    if prep is not None:
        a.delta, a.mu_bf16, a.delta_bf16 = _ptr(prep["delta"]), _ptr(prep["mu_bf16"]), _ptr(prep["delta_bf16"])
    a.b_draw, a.y = b.data_ptr(), y.data_ptr()
    L.check(lib.bnn_flipout_fwd(C.byref(a), _stream()), "bnn_flipout_fwd")
    return y


def flipout_bwd(x, gy, y, w_mu, w_rho, b_mu, b_rho, eps_w, eps_b, *, n_samples: int, n_draws: int, prior: PriorSpec, relu: bool,
                seed: int = 0, layer_id: int = 0, sample_offset: int = 0, sample_counter=None, row_offset: int = 0,
                g_log_prior=None, g_log_q=None, want_gx: bool = True, out=None):
    """bnn_flipout_bwd: (g_w_mu, g_w_rho, g_b_mu, g_b_rho, g_x [S, batch, in] | None).  `out`: four tensors to write the
    parameter gradients into."""
    lib = L.load()
    require_device(x, gy, w_mu)
    S, D = int(n_samples), int(n_draws)
    N, K = w_mu.shape
    x, gy = _f32c(x, "x"), _f32c(gy, "gy")
    B = x.shape[-2]
    dev = x.device
    g = list(out) if out is not None else [torch.empty_like(t, dtype=torch.float32) for t in (w_mu, w_rho, b_mu, b_rho)]
    gx = torch.empty((S, B, K), dtype=torch.float32, device=dev) if want_gx else None
    ws = torch.empty(lib.bnn_flipout_bwd_workspace_bytes(S, B, K, N) // 4, dtype=torch.float32, device=dev)
    keep = [_f32c(t, "parameter") for t in (w_mu, w_rho, b_mu, b_rho, eps_w, eps_b)]
    glp = None if g_log_prior is None else _f32c(g_log_prior, "g_log_prior")
    glq = None if g_log_q is None else _f32c(g_log_q, "g_log_q")
    a = L.FlipoutBwdArgs()
    a.struct_bytes = C.sizeof(L.FlipoutBwdArgs)
    a.n_samples, a.n_draws, a.batch, a.in_features, a.out_features = S, D, B, K, N
    a.x_per_sample, a.relu = int(x.dim() == 3), int(bool(relu))
    a.layer_id, a.sample_offset, a.row_offset = layer_id, sample_offset & 0xFFFFFFFF, row_offset & 0xFFFFFFFF
    a.seed, a.sample_counter = seed & 0xFFFFFFFFFFFFFFFF, _ptr(sample_counter)
    a.x, a.gy, a.y = x.data_ptr(), gy.data_ptr(), _ptr(y) if relu else None
    a.w_mu, a.w_rho, a.b_mu, a.b_rho, a.eps_w, a.eps_b = (t.data_ptr() for t in keep)
    a.prior = prior.c()
    a.g_log_prior, a.g_log_q = _ptr(glp), _ptr(glq)
    a.g_w_mu, a.g_w_rho, a.g_b_mu, a.g_b_rho = (t.data_ptr() for t in g)
    a.g_x, a.workspace, a.workspace_bytes = _ptr(gx), ws.data_ptr(), ws.numel() * 4
    L.check(lib.bnn_flipout_bwd(C.byref(a), _stream()), "bnn_flipout_bwd")
    return g[0], g[1], g[2], g[3], gx


# ---------------------------------------------------------------------------------------------- F17: diagonal Laplace
LAPLACE_CURVATURES = {"ggn": L.LAPLACE_GGN, "empirical": L.LAPLACE_EMPIRICAL}


def _lap_f32(t, name: str, shape=None):
    """A contiguous float32 device tensor (of `shape`), or None."""
    if t is None:
        return None
    require_device(t)
    if t.dtype != torch.float32 or not t.is_contiguous() or (shape is not None and tuple(t.shape) != tuple(shape)):
        want = "" if shape is None else f" of shape {tuple(shape)}"
        raise BnnHipError(f"laplace: {name} must be a contiguous float32 tensor{want}, got {tuple(t.shape)} {t.dtype}")
    return t


def _lap_f64(t, name: str, numel: int):
    require_device(t)
    if t.dtype != torch.float64 or not t.is_contiguous() or t.numel() != numel:
        raise BnnHipError(f"laplace: {name} must be a contiguous float64 tensor of {numel} elements")
    return t


def laplace_rows(batch: int, classes: int, curvature: str) -> int:
    """The virtual rows R of a minibatch: batch * classes under the GGN (one per class), batch under the empirical Fisher."""
    if curvature not in LAPLACE_CURVATURES:
        raise BnnHipError(f"laplace: curvature must be one of {tuple(LAPLACE_CURVATURES)}, got {curvature!r}")
    return batch * classes if curvature == "ggn" else batch


def laplace_seed(logits, target, mode: str, *, curvature: str = "ggn", sigma: float = 1.0, gy=None, record):
    """F17 bnn_laplace_seed: the output-layer deltas gy [R, C] (virtual row c * B + n under the GGN) of logits [B, C], and
    record (float64 [2]) += (sum of log-likelihoods, B).  `target`: int64 [B] (classification) or float32 of B * C elements
    (regression); None under the GGN leaves record[0] alone."""
    lib = L.load()
    logits = _lap_f32(logits, "logits")
    if logits.dim() != 2:
        raise BnnHipError(f"laplace_seed: logits must be [batch, classes], got {tuple(logits.shape)}")
    B, Cc = logits.shape
    R = laplace_rows(B, Cc, curvature)
    if mode not in ("classification", "regression"):
        raise BnnHipError(f"laplace_seed: unknown mode {mode!r}")
    if target is not None:
        require_device(target)
        if mode == "classification" and (target.dtype != torch.int64 or target.numel() != B):
            raise BnnHipError("laplace_seed: classification targets must be int64 labels, one per row")
        if mode == "regression" and (target.dtype != torch.float32 or target.numel() != B * Cc):
            raise BnnHipError(f"laplace_seed: regression targets must be float32 with {B * Cc} elements")
        target = target if target.is_contiguous() else target.contiguous()
    gy = torch.empty((R, Cc), dtype=torch.float32, device=logits.device) if gy is None else _lap_f32(gy, "gy", (R, Cc))
    a = L.LaplaceSeedArgs()
    a.struct_bytes = C.sizeof(L.LaplaceSeedArgs)
    a.batch, a.classes = B, Cc
    a.loss_mode = L.NLL_CLASSIFICATION if mode == "classification" else L.NLL_REGRESSION
    a.curvature, a.sigma = LAPLACE_CURVATURES[curvature], float(sigma)
    a.logits, a.target, a.gy = logits.data_ptr(), _ptr(target), gy.data_ptr()
    a.record = _lap_f64(record, "record", L.LAPLACE_RECORD_DOUBLES).data_ptr()
    L.check(lib.bnn_laplace_seed(C.byref(a), _stream()), "bnn_laplace_seed")
    return gy


def laplace_layer(x, gy, w, *, f_w, f_b=None, g_x=None, y=None, gx_mask: bool = False, s_out=None,
                  math_mode: int = L.MATH_F32):
    """F17 bnn_laplace_layer: one Linear -> [ReLU] group.  x [B, in], gy [R, out] (R a multiple of B), the saved output
    y [B, out] (gz = y > 0 ? gy : 0) or None; f_w [out, in] += S^T x^2, f_b [out] += colsum(S) with S[n, o] the sum over
    the virtual rows of data row n of gz^2; g_x [R, in] = gz w, times (x > 0) when gx_mask; s_out [B, out] = S."""
    lib = L.load()
    x = _lap_f32(x, "x")
    B, K = x.shape
    N = w.shape[0]
    gy = _lap_f32(gy, "gy")
    R = gy.shape[0]
    if gy.dim() != 2 or R % B != 0:
        raise BnnHipError(f"laplace_layer: gy must be [rows, out] with rows a multiple of the batch {B}, got {tuple(gy.shape)}")
    _lap_f32(gy, "gy", (R, N)), _lap_f32(w, "w", (N, K)), _lap_f32(f_w, "f_w", (N, K)), _lap_f32(f_b, "f_b", (N,))
    _lap_f32(g_x, "g_x", (R, K)), _lap_f32(y, "y", (B, N)), _lap_f32(s_out, "s_out", (B, N))
    a = L.LaplaceLayerArgs()
    a.struct_bytes = C.sizeof(L.LaplaceLayerArgs)
    a.batch, a.rows, a.in_features, a.out_features = B, R, K, N
    a.math, a.gx_mask = _exact_unless_bf16(math_mode), int(bool(gx_mask))
    a.x, a.gy, a.y, a.w = x.data_ptr(), gy.data_ptr(), _ptr(y), w.data_ptr()
    a.f_w, a.f_b, a.g_x, a.s_out = f_w.data_ptr(), _ptr(f_b), _ptr(g_x), _ptr(s_out)
    L.check(lib.bnn_laplace_layer(C.byref(a), _stream()), "bnn_laplace_layer")


def _lap_pairs(a, params, curvs):
    n = len(params)
    if not 1 <= n <= L.LAPLACE_MAX_TENSORS or len(curvs) != n:
        raise BnnHipError(f"laplace: between 1 and {L.LAPLACE_MAX_TENSORS} (parameter, curvature) pairs, got {n} / {len(curvs)}")
    a.n_tensors = n
    for j, (p, f) in enumerate(zip(params, curvs)):
        _lap_f32(p, "parameter"), _lap_f32(f, "curvature", p.shape)
        a.param[j], a.curv[j], a.numel[j] = p.data_ptr(), f.data_ptr(), p.numel()


def laplace_evidence(params, curvs, precisions, *, record, log_evidence=None, best_index=None, best=None, workspace=None):
    """F17 bnn_laplace_evidence: the Laplace log marginal likelihood at every candidate prior precision (host floats), in
    fp64 on the device -> (log_evidence float64 [G], best_index int32 [1], best float64 [2] = (maximum, its precision)).
    Nothing is read back."""
    lib = L.load()
    taus = [float(t) for t in precisions]
    G = len(taus)
    if not 1 <= G <= L.LAPLACE_MAX_PRECISIONS:
        raise BnnHipError(f"laplace_evidence: between 1 and {L.LAPLACE_MAX_PRECISIONS} candidate precisions, got {G}")
    if not all(0.0 < t < math.inf for t in taus):
        raise BnnHipError("laplace_evidence: prior precisions must be positive and finite")
    a = L.LaplaceEvidenceArgs()
    a.struct_bytes = C.sizeof(L.LaplaceEvidenceArgs)
    _lap_pairs(a, params, curvs)
    a.n_precisions = G
    for g, t in enumerate(taus):
        a.precision[g] = t
    dev = params[0].device
    need = lib.bnn_laplace_evidence_workspace_bytes(C.byref(a))
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty(need // 8, dtype=torch.float64, device=dev)
    log_evidence = torch.empty(G, dtype=torch.float64, device=dev) if log_evidence is None else _lap_f64(log_evidence, "log_evidence", G)
    best_index = torch.zeros(1, dtype=torch.int32, device=dev) if best_index is None else _typed(best_index, torch.int32, "best_index", 1)
    best = torch.zeros(2, dtype=torch.float64, device=dev) if best is None else _lap_f64(best, "best", 2)
    a.record = _lap_f64(record, "record", L.LAPLACE_RECORD_DOUBLES).data_ptr()
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    a.log_evidence, a.best_index, a.best = log_evidence.data_ptr(), best_index.data_ptr(), best.data_ptr()
    L.check(lib.bnn_laplace_evidence(C.byref(a), _stream()), "bnn_laplace_evidence")
    return log_evidence, best_index, best


def laplace_posterior(params, curvs, mus, rhos, *, precision=None, precision_device=None):
    """F17 bnn_laplace_posterior: mu = w, rho = softplus^-1((F + tau)^-1/2) for every tensor in one launch; tau a host float
    or a one-element float64 device tensor (best[1:2] of laplace_evidence)."""
    lib = L.load()
    a = L.LaplacePosteriorArgs()
    a.struct_bytes = C.sizeof(L.LaplacePosteriorArgs)
    _lap_pairs(a, params, curvs)
    if len(mus) != len(params) or len(rhos) != len(params):
        raise BnnHipError("laplace_posterior: one (mu, rho) pair per parameter")
    for j, (p, m, r) in enumerate(zip(params, mus, rhos)):
        _lap_f32(m, "mu", p.shape), _lap_f32(r, "rho", p.shape)
        a.mu[j], a.rho[j] = m.data_ptr(), r.data_ptr()
    if precision_device is not None:
        a.precision, a.precision_device = 1.0, _lap_f64(precision_device, "precision_device", 1).data_ptr()
    else:
        if precision is None or not 0.0 < float(precision) < math.inf:
            raise BnnHipError(f"laplace_posterior: the prior precision must be positive and finite, got {precision!r}")
        a.precision, a.precision_device = float(precision), None
    L.check(lib.bnn_laplace_posterior(C.byref(a), _stream()), "bnn_laplace_posterior")


# ---------------------------------------------------------------------------------------------- F18: the GLM predictive
GLM_TILE = 64


def glm_pairs(classes: int) -> int:
    """The pairs c <= c' of a covariance row: pair = c' (c' + 1) / 2 + c."""
    if not 1 <= int(classes) <= L.LAPLACE_GLM_MAX_CLASSES:
        raise BnnHipError(f"laplace_glm: between 1 and {L.LAPLACE_GLM_MAX_CLASSES} outputs (BNN_LAPLACE_GLM_MAX_CLASSES), got {classes}")
    return int(classes) * (int(classes) + 1) // 2


def glm_tiles(out_features: int) -> int:
    return (int(out_features) + GLM_TILE - 1) // GLM_TILE


def _glm_precision(a, precision, precision_device, what: str):
    if precision_device is not None:
        a.precision, a.precision_device = 1.0, _lap_f64(precision_device, "precision_device", 1).data_ptr()
    else:
        if precision is None or not 0.0 < float(precision) < math.inf:
            raise BnnHipError(f"{what}: the prior precision must be positive and finite, got {precision!r}")
        a.precision, a.precision_device = float(precision), None


def laplace_glm_layer(x, gy, w, *, f_w, f_b, cov_part=None, g_x=None, y=None, gx_mask: bool = False, v_out=None,
                      precision=None, precision_device=None, math_mode: int = L.MATH_F32):
    """F18 bnn_laplace_glm_layer: one Linear -> [ReLU] group of the linearised predictive.  x [B, in], gy [R, out] (R = B * C,
    C <= 16), the saved output y [B, out] or None, the curvature (f_w [out, in], f_b [out]) and tau (a host float, or a
    one-element float64 device tensor); cov_part [ceil(out / 64), B, C (C + 1) / 2] receives the tile partials of
    sum_o gz_c gz_c' V with V = x^2 . (1 / (f_w + tau))^T + 1 / (f_b + tau); g_x [R, in] = gz w as laplace_layer's;
    v_out [B, out] = V.  Returns cov_part."""
    lib = L.load()
    x = _lap_f32(x, "x")
    if x.dim() != 2:
        raise BnnHipError(f"laplace_glm_layer: x must be [batch, in], got {tuple(x.shape)}")
    B, K = x.shape
    N = w.shape[0]
    gy = _lap_f32(gy, "gy")
    R = gy.shape[0]
    if gy.dim() != 2 or R % B != 0:
        raise BnnHipError(f"laplace_glm_layer: gy must be [rows, out] with rows a multiple of the batch {B}, got {tuple(gy.shape)}")
    P = glm_pairs(R // B)
    _lap_f32(gy, "gy", (R, N)), _lap_f32(w, "w", (N, K)), _lap_f32(f_w, "f_w", (N, K)), _lap_f32(f_b, "f_b", (N,))
    _lap_f32(g_x, "g_x", (R, K)), _lap_f32(y, "y", (B, N)), _lap_f32(v_out, "v_out", (B, N))
    if f_w is None or f_b is None:
        raise BnnHipError("laplace_glm_layer: the curvature (f_w, f_b) is needed")
    shape = (glm_tiles(N), B, P)
    cov_part = torch.empty(shape, dtype=torch.float32, device=x.device) if cov_part is None else _lap_f32(cov_part, "cov_part", shape)
    a = L.LaplaceGlmLayerArgs()
    a.struct_bytes = C.sizeof(L.LaplaceGlmLayerArgs)
    a.batch, a.rows, a.in_features, a.out_features = B, R, K, N
    a.math, a.gx_mask = _exact_unless_bf16(math_mode), int(bool(gx_mask))
    _glm_precision(a, precision, precision_device, "laplace_glm_layer")
    a.x, a.gy, a.y, a.w = x.data_ptr(), gy.data_ptr(), _ptr(y), w.data_ptr()
    a.f_w, a.f_b, a.g_x, a.cov_part, a.v_out = f_w.data_ptr(), f_b.data_ptr(), _ptr(g_x), cov_part.data_ptr(), _ptr(v_out)
    L.check(lib.bnn_laplace_glm_layer(C.byref(a), _stream()), "bnn_laplace_glm_layer")
    return cov_part


class GlmMoments(NamedTuple):
    """What bnn_laplace_glm_finish writes: cov [B, C, C], var [B, C], chol [B, C, C] and the mode's closed-form summaries
    (classification probs / preds / entropy; regression predictive_variance / quantiles [Q, B, C])."""
    cov: torch.Tensor
    var: torch.Tensor
    chol: torch.Tensor
    probs: Optional[torch.Tensor] = None
    preds: Optional[torch.Tensor] = None
    entropy: Optional[torch.Tensor] = None
    predictive_variance: Optional[torch.Tensor] = None
    quantiles: Optional[torch.Tensor] = None


def normal_quantiles(levels) -> tuple:
    """z_q = Phi^-1(q) in fp64 for checked quantile levels; -inf / +inf at 0 / 1."""
    import statistics
    nd = statistics.NormalDist()
    return tuple(-math.inf if q == 0.0 else math.inf if q == 1.0 else nd.inv_cdf(q) for q in quantile_levels(levels))


def glm_buffers(mode: str, B: int, Cc: int, device, n_quantiles: int = 0) -> GlmMoments:
    f = dict(dtype=torch.float32, device=device)
    base = dict(cov=torch.empty((B, Cc, Cc), **f), var=torch.empty((B, Cc), **f), chol=torch.empty((B, Cc, Cc), **f))
    if mode == "classification":
        return GlmMoments(probs=torch.empty((B, Cc), **f), preds=torch.empty(B, dtype=torch.int64, device=device),
                          entropy=torch.empty(B, **f), **base)
    if mode == "regression":
        return GlmMoments(predictive_variance=torch.empty((B, Cc), **f),
                          quantiles=torch.empty((n_quantiles, B, Cc), **f) if n_quantiles else None, **base)
    raise Exception("Training mode must be either 'regression' or 'classification'")


def laplace_glm_finish(parts, mean, mode: str, *, sigma: float = 1.0, quantiles=(), out: Optional[GlmMoments] = None,
                       sample_counter=None, n_samples: int = 0) -> GlmMoments:
    """F18 bnn_laplace_glm_finish: `parts` the cov_part tensors of the layers ([tiles, B, pairs] each, summed in list order),
    `mean` [B, C] the network's output -> GlmMoments.  `quantiles`: levels in [0, 1] (regression).  `sample_counter`: a uint32
    (int32 storage) device word that the launch advances by `n_samples`."""
    lib = L.load()
    mean = _lap_f32(mean, "mean")
    if mean.dim() != 2:
        raise BnnHipError(f"laplace_glm_finish: mean must be [batch, outputs], got {tuple(mean.shape)}")
    B, Cc = mean.shape
    P = glm_pairs(Cc)
    parts = list(parts)
    if not 1 <= len(parts) <= L.LAPLACE_GLM_MAX_LAYERS:
        raise BnnHipError(f"laplace_glm_finish: between 1 and {L.LAPLACE_GLM_MAX_LAYERS} layers, got {len(parts)}")
    if mode not in ("classification", "regression"):
        raise Exception("Training mode must be either 'regression' or 'classification'")
    z = normal_quantiles(quantiles) if mode == "regression" else ()
    if mode == "regression" and not 0.0 < float(sigma) < math.inf:
        raise BnnHipError(f"laplace_glm_finish: sigma must be positive and finite, got {sigma!r}")
    if int(n_samples) < 0:
        raise BnnHipError("laplace_glm_finish: n_samples must be >= 0")
    if out is None:
        out = glm_buffers(mode, B, Cc, mean.device, len(z))
    want = dict(cov=(B, Cc, Cc), var=(B, Cc), chol=(B, Cc, Cc), probs=(B, Cc), preds=(B,), entropy=(B,),
                predictive_variance=(B, Cc), quantiles=(len(z), B, Cc))
    for name, t in zip(out._fields, out):
        if t is None:
            continue
        require_device(t)
        dt = torch.int64 if name == "preds" else torch.float32
        if tuple(t.shape) != want[name] or t.dtype != dt or not t.is_contiguous():
            raise BnnHipError(f"laplace_glm_finish: out.{name} must be a contiguous {dt} tensor of shape {want[name]}")
    if z and out.quantiles is None:
        raise BnnHipError("laplace_glm_finish: quantile levels need out.quantiles")
    a = L.LaplaceGlmFinishArgs()
    a.struct_bytes = C.sizeof(L.LaplaceGlmFinishArgs)
    a.batch, a.classes, a.n_layers = B, Cc, len(parts)
    a.mode = L.NLL_CLASSIFICATION if mode == "classification" else L.NLL_REGRESSION
    a.n_quantiles, a.n_samples, a.sigma = len(z), int(n_samples), float(sigma)
    for i, v in enumerate(z):
        a.z[i] = v
    for i, t in enumerate(parts):
        t = _lap_f32(t, "cov_part")
        if t.dim() != 3 or t.shape[0] < 1 or tuple(t.shape[1:]) != (B, P):
            raise BnnHipError(f"laplace_glm_finish: a cov_part must be [tiles, {B}, {P}], got {tuple(t.shape)}")
        a.cov_part[i], a.tiles[i] = t.data_ptr(), t.shape[0]
    a.mean, a.cov, a.var, a.chol = mean.data_ptr(), out.cov.data_ptr(), out.var.data_ptr(), out.chol.data_ptr()
    if mode == "classification":
        a.probs, a.preds, a.entropy = _ptr(out.probs), _ptr(out.preds), _ptr(out.entropy)
    else:
        a.predictive_variance, a.quantiles = _ptr(out.predictive_variance), _ptr(out.quantiles) if z else None
    if sample_counter is not None:
        a.sample_counter = _typed(sample_counter, torch.int32, "sample_counter", 1).data_ptr()
    L.check(lib.bnn_laplace_glm_finish(C.byref(a), _stream()), "bnn_laplace_glm_finish")
    return out


def laplace_glm_sample(mean, chol, n_samples: int, *, seed: int, sample_base: int = 0, sample_counter=None, out=None):
    """F18 bnn_laplace_glm_sample: logits [S, B, C] = mean + chol . eps, eps from the Philox stream (5, 1) at the global
    sample indices sample_base + (*sample_counter - S, when a counter is given) + s."""
    lib = L.load()
    mean = _lap_f32(mean, "mean")
    if mean.dim() != 2:
        raise BnnHipError(f"laplace_glm_sample: mean must be [batch, outputs], got {tuple(mean.shape)}")
    B, Cc = mean.shape
    glm_pairs(Cc)
    S = int(n_samples)
    if S < 1:
        raise BnnHipError(f"laplace_glm_sample: at least one sample, got {n_samples}")
    _lap_f32(chol, "chol", (B, Cc, Cc))
    if chol is None:
        raise BnnHipError("laplace_glm_sample: chol is needed")
    out = torch.empty((S, B, Cc), dtype=torch.float32, device=mean.device) if out is None else _lap_f32(out, "logits", (S, B, Cc))
    a = L.LaplaceGlmSampleArgs()
    a.struct_bytes = C.sizeof(L.LaplaceGlmSampleArgs)
    a.n_samples, a.batch, a.classes = S, B, Cc
    a.seed, a.sample_base = int(seed) & 0xFFFFFFFFFFFFFFFF, int(sample_base) & 0xFFFFFFFF
    a.mean, a.chol, a.logits = mean.data_ptr(), chol.data_ptr(), out.data_ptr()
    if sample_counter is not None:
        a.sample_counter = _typed(sample_counter, torch.int32, "sample_counter", 1).data_ptr()
    L.check(lib.bnn_laplace_glm_sample(C.byref(a), _stream()), "bnn_laplace_glm_sample")
    return out


# ---------------------------------------------------------------------------------------------------------------- F19 SG-MCMC
def sgmcmc_noise(seed: int, tensor: int, step: int, numel: int, device) -> torch.Tensor:
    """F19 bnn_sgmcmc_noise: the SG-MCMC noise stream of parameter tensor `tensor` at chain step `step`, materialised:
    float32[numel] (counter (i >> 2, step, tensor, 3), slot i & 3)."""
    lib = L.load()
    if torch.device(device).type != "cuda":
        raise BnnHipError("bnn_hip.sgmcmc_noise needs a ROCm device")
    if not 0 <= int(tensor) < L.SGMCMC_MAX_TENSORS or int(numel) < 1:
        raise BnnHipError(f"sgmcmc_noise: tensor must lie in [0, {L.SGMCMC_MAX_TENSORS}) and numel be >= 1")
    out = torch.empty(int(numel), dtype=torch.float32, device=device)
    L.check(lib.bnn_sgmcmc_noise(out.data_ptr(), int(seed) & 0xFFFFFFFFFFFFFFFF, int(tensor), int(step) & 0xFFFFFFFF, int(numel),
                                 _stream()), "bnn_sgmcmc_noise")
    return out


def bank_layout(numels: Sequence[int]) -> tuple:
    """(offsets, stride) of a weight bank's member: every tensor starts at a multiple of 64 elements."""
    offs, tot = [], 0
    for n in numels:
        offs.append(tot)
        tot += (int(n) + 63) // 64 * 64
    return tuple(offs), tot


def sgmcmc_step(params, grads, *, table: torch.Tensor, step: torch.Tensor, ticket: torch.Tensor, grad_scale: float, tau: float,
                eps_mode: int = L.EPS_PHILOX, seed: int = 0, momenta=None, noise=None, burn_in: int = 0, collected=None,
                bank: Optional[torch.Tensor] = None):
    """F19 bnn_sgmcmc_step: one SGLD (momenta None) / SGHMC step over lists of fp32 tensors in one launch.  `table`: device
    float32 [L, 4] rows (a, b, c, collect flag); `step`, `collected`: one-element int32 device words (read as uint32), `ticket`
    16 zeroed int32 words; `noise`: one tensor per parameter (EPS_MEMORY).  `bank`: float32 [capacity, stride] with the
    stride of bank_layout -- the step files its result into member collected % capacity when its table row says so."""
    lib = L.load()
    n = len(params)
    if not 1 <= n <= L.SGMCMC_MAX_TENSORS:
        raise BnnHipError(f"sgmcmc_step: between 1 and {L.SGMCMC_MAX_TENSORS} parameter tensors, got {n}")
    if len(grads) != n or (momenta is not None and len(momenta) != n) or (eps_mode == L.EPS_MEMORY and (noise is None or len(noise) != n)):
        raise BnnHipError("sgmcmc_step: one gradient (momentum, noise) tensor per parameter")
    require_device(table, step, ticket, collected, bank)
    if table.dtype != torch.float32 or table.dim() != 2 or table.shape[1] != L.SGMCMC_TABLE_COLS or not table.is_contiguous() or \
            table.shape[0] < 1:
        raise BnnHipError(f"sgmcmc_step: table must be a contiguous float32 [L, {L.SGMCMC_TABLE_COLS}] tensor")
    _typed(step, torch.int32, "step", 1)
    _typed(ticket, torch.int32, "ticket", 16)
    a = L.SgmcmcArgs()
    a.struct_bytes = C.sizeof(L.SgmcmcArgs)
    a.n_tensors = n
    keep = [table, step, ticket, collected, bank]
    for j in range(n):
        ts = [params[j], grads[j]] + ([momenta[j]] if momenta is not None else []) + ([noise[j]] if eps_mode == L.EPS_MEMORY else [])
        for t in ts:
            require_device(t)
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != params[j].numel():
                raise BnnHipError("sgmcmc_step: parameters, gradients, momenta and noise must be contiguous float32 of one size")
        keep += ts
        a.param[j], a.grad[j], a.numel[j] = params[j].data_ptr(), grads[j].data_ptr(), params[j].numel()
        if momenta is not None:
            a.momentum[j] = momenta[j].data_ptr()
        if eps_mode == L.EPS_MEMORY:
            a.noise[j] = noise[j].data_ptr()
    a.grad_scale, a.tau, a.eps_mode = float(grad_scale), float(tau), int(eps_mode)
    a.table_rows, a.table = table.shape[0], table.data_ptr()
    a.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    a.step, a.ticket, a.burn_in = step.data_ptr(), ticket.data_ptr(), int(burn_in) & 0xFFFFFFFF
    if bank is not None:
        stride = bank_layout([p.numel() for p in params])[1]
        if bank.dtype != torch.float32 or bank.dim() != 2 or bank.shape[1] != stride or not bank.is_contiguous() or bank.shape[0] < 1:
            raise BnnHipError(f"sgmcmc_step: the bank must be a contiguous float32 [capacity, {stride}] tensor")
        if collected is None:
            raise BnnHipError("sgmcmc_step: a bank needs its `collected` word")
        a.collected = _typed(collected, torch.int32, "collected", 1).data_ptr()
        a.bank, a.capacity = bank.data_ptr(), bank.shape[0]
    a._keep = keep
    L.check(lib.bnn_sgmcmc_step(C.byref(a), _stream()), "bnn_sgmcmc_step")


# ---------------------------------------------------------------------------------------------------------------- F22 SWAG
def swag_collects(step: int, start: int, every: int) -> bool:
    """bnn_swag_step's predicate on the uint32 step word: k >= start and (k - start + 1) % every == 0."""
    k, start = int(step) & 0xFFFFFFFF, int(start) & 0xFFFFFFFF
    return k >= start and (k - start + 1) % int(every) == 0


def swag_coefficients(scale: float, low_rank: bool = True) -> tuple:
    """(c_d, c_lr) of bnn_swag_sample, formed in fp64 and rounded once: c_d = sqrt(scale / 2) with the low-rank term and
    sqrt(scale) without; c_lr[e] = sqrt(scale / (2 (e - 1))) for e = 2 .. SWAG_MAX_RANK, c_lr[0] = c_lr[1] = 0 (all 0
    without the low-rank term)."""
    import numpy as np
    scale = float(scale)
    if not 0.0 <= scale < float("inf"):
        raise BnnHipError(f"swag: scale must be finite and >= 0, got {scale!r}")
    c_lr = np.zeros(L.SWAG_MAX_RANK + 1, dtype=np.float64)
    if low_rank:
        e = np.arange(2, L.SWAG_MAX_RANK + 1, dtype=np.float64)
        c_lr[2:] = np.sqrt(scale / (2.0 * (e - 1.0)))
    return float(np.float32(math.sqrt(scale / 2.0 if low_rank else scale))), c_lr.astype(np.float32)


def _swag_moments(name, numels, mean, m2, dev, rank):
    stride = bank_layout(numels)[1]
    require_device(mean, m2, dev)
    for t, nm in ((mean, "mean"), (m2, "m2")):
        if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (stride,):
            raise BnnHipError(f"{name}: {nm} must be a contiguous float32 [{stride}] tensor (the bank's layout)")
    if rank > 0 and (dev is None or dev.dtype != torch.float32 or not dev.is_contiguous() or tuple(dev.shape) != (rank, stride)):
        raise BnnHipError(f"{name}: dev must be a contiguous float32 [{rank}, {stride}] tensor")
    return stride


def swag_step(params, grads, *, lr: float, momentum: float = 0.0, weight_decay: float = 0.0, lr_device=None, momenta=None,
              start: int = 0, every: int = 1, mean: torch.Tensor, m2: torch.Tensor, dev: Optional[torch.Tensor],
              step: torch.Tensor, count: torch.Tensor, ticket: torch.Tensor):
    """F22 bnn_swag_step: one torch.optim.SGD step (momenta None: no momentum buffer) over lists of fp32 tensors in one
    launch; when the step word k has k >= start and (k - start + 1) % every == 0 the launch also folds the new iterate into
    `mean`, `m2` (Welford) and row count % rank of `dev` ([rank, stride]; None: rank 0).  `step`, `count`: one-element int32
    device words (read as uint32), `ticket` 16 zeroed int32 words."""
    lib = L.load()
    n = len(params)
    if not 1 <= n <= L.SGMCMC_MAX_TENSORS:
        raise BnnHipError(f"swag_step: between 1 and {L.SGMCMC_MAX_TENSORS} parameter tensors, got {n}")
    if len(grads) != n or (momenta is not None and len(momenta) != n):
        raise BnnHipError("swag_step: one gradient (momentum) tensor per parameter")
    rank = 0 if dev is None else int(dev.shape[0])
    if rank > L.SWAG_MAX_RANK or int(every) < 1 or int(start) < 0:
        raise BnnHipError(f"swag_step: rank <= {L.SWAG_MAX_RANK}, every >= 1 and start >= 0 are required")
    require_device(step, count, ticket, lr_device)
    _swag_moments("swag_step", [p.numel() for p in params], mean, m2, dev, rank)
    a = L.SwagStepArgs()
    a.struct_bytes = C.sizeof(L.SwagStepArgs)
    a.n_tensors = n
    keep = [mean, m2, dev, step, count, ticket, lr_device]
    for j in range(n):
        ts = [params[j], grads[j]] + ([momenta[j]] if momenta is not None else [])
        for t in ts:
            require_device(t)
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != params[j].numel():
                raise BnnHipError("swag_step: parameters, gradients and momenta must be contiguous float32 of one size")
        keep += ts
        a.param[j], a.grad[j], a.numel[j] = params[j].data_ptr(), grads[j].data_ptr(), params[j].numel()
        if momenta is not None:
            a.momentum[j] = momenta[j].data_ptr()
    a.lr, a.momentum_factor, a.weight_decay, a.lr_device = float(lr), float(momentum), float(weight_decay), _ptr(lr_device)
    a.start, a.every, a.rank = int(start) & 0xFFFFFFFF, int(every), rank
    a.mean, a.m2, a.dev = mean.data_ptr(), m2.data_ptr(), _ptr(dev)
    a.step = _typed(step, torch.int32, "step", 1).data_ptr()
    a.count = _typed(count, torch.int32, "count", 1).data_ptr()
    a.ticket = _typed(ticket, torch.int32, "ticket", 16).data_ptr()
    a._keep = keep
    L.check(lib.bnn_swag_step(C.byref(a), _stream()), "bnn_swag_step")


def swag_sample(numels: Sequence[int], mean: torch.Tensor, m2: torch.Tensor, dev: Optional[torch.Tensor], count: torch.Tensor,
                bank: torch.Tensor, *, members: int, first: int = 0, scale: float = 1.0, low_rank: bool = True,
                var_clamp: float = 1e-30, eps_mode: int = L.EPS_PHILOX, seed: int = 0, sample_base: int = 0, z1=None, z2=None):
    """F22 bnn_swag_sample: members first .. first + members - 1 of `bank` (float32 [capacity, stride]) drawn from the SWAG
    Gaussian in one launch, members <= SWAG_MAX_MEMBERS: theta = mean + c_d sqrt(max(m2 / n, var_clamp)) z1 [+ c_lr[Keff]
    sum_j dev[j] z2[j]], n = the device word `count`, Keff = min(n, rank).  Draw j of the launch is global draw
    sample_base + j of the seed's streams.  EPS_MEMORY: z1 [members, stride], z2 [members, rank]."""
    lib = L.load()
    numels = [int(v) for v in numels]
    if not 1 <= len(numels) <= L.SGMCMC_MAX_TENSORS:
        raise BnnHipError(f"swag_sample: between 1 and {L.SGMCMC_MAX_TENSORS} parameter tensors, got {len(numels)}")
    rank = 0 if dev is None else int(dev.shape[0])
    m, first = int(members), int(first)
    if low_rank and rank == 0:
        raise BnnHipError("swag_sample: the low-rank term needs deviation rows (rank >= 1); pass low_rank=False for SWAG-Diagonal")
    if rank > L.SWAG_MAX_RANK or not 1 <= m <= L.SWAG_MAX_MEMBERS or not float(var_clamp) >= 0.0:
        raise BnnHipError(f"swag_sample: rank <= {L.SWAG_MAX_RANK}, 1 <= members <= {L.SWAG_MAX_MEMBERS} and var_clamp >= 0 are required")
    stride = _swag_moments("swag_sample", numels, mean, m2, dev, rank)
    require_device(count, bank, z1, z2)
    if bank.dtype != torch.float32 or bank.dim() != 2 or bank.shape[1] != stride or not bank.is_contiguous():
        raise BnnHipError(f"swag_sample: the bank must be a contiguous float32 [capacity, {stride}] tensor")
    if first < 0 or first + m > bank.shape[0]:
        raise BnnHipError(f"swag_sample: members [{first}, {first + m}) outside the bank's {bank.shape[0]}")
    a = L.SwagSampleArgs()
    a.struct_bytes = C.sizeof(L.SwagSampleArgs)
    a.n_tensors = len(numels)
    for j, v in enumerate(numels):
        a.numel[j] = v
    a.rank, a.members, a.first, a.capacity = rank, m, first, bank.shape[0]
    a.low_rank, a.eps_mode = 1 if low_rank else 0, int(eps_mode)
    c_d, c_lr = swag_coefficients(scale, bool(low_rank))
    a.c_d, a.var_clamp = c_d, float(var_clamp)
    for e in range(L.SWAG_MAX_RANK + 1):
        a.c_lr[e] = float(c_lr[e])
    a.sample_base, a.seed = int(sample_base) & 0xFFFFFFFF, int(seed) & 0xFFFFFFFFFFFFFFFF
    a.mean, a.m2, a.dev = mean.data_ptr(), m2.data_ptr(), _ptr(dev) if low_rank else None
    a.count, a.bank = _typed(count, torch.int32, "count", 1).data_ptr(), bank.data_ptr()
    if eps_mode == L.EPS_MEMORY:
        if z1 is None or z1.dtype != torch.float32 or not z1.is_contiguous() or tuple(z1.shape) != (m, stride):
            raise BnnHipError(f"swag_sample: z1 must be a contiguous float32 [{m}, {stride}] tensor")
        a.z1 = z1.data_ptr()
        if low_rank:
            if z2 is None or z2.dtype != torch.float32 or not z2.is_contiguous() or tuple(z2.shape) != (m, rank):
                raise BnnHipError(f"swag_sample: z2 must be a contiguous float32 [{m}, {rank}] tensor")
            a.z2 = z2.data_ptr()
    a._keep = [mean, m2, dev, count, bank, z1, z2]
    L.check(lib.bnn_swag_sample(C.byref(a), _stream()), "bnn_swag_sample")
    return bank


# ---------------------------------------------------------------------------------------------------------------- F24 IVON
def _ivon_flat(name, what, t, stride, rows=None):
    shape = (stride,) if rows is None else (rows, stride)
    if t is None or t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shape:
        raise BnnHipError(f"{name}: {what} must be a contiguous float32 {list(shape)} tensor (the bank's layout)")
    return t.data_ptr()


def _ivon_tensors(name, a, params, grads):
    n = len(params)
    if not 1 <= n <= L.SGMCMC_MAX_TENSORS:
        raise BnnHipError(f"{name}: between 1 and {L.SGMCMC_MAX_TENSORS} parameter tensors, got {n}")
    if grads is not None and len(grads) != n:
        raise BnnHipError(f"{name}: one gradient tensor per parameter")
    a.n_tensors = n
    keep = []
    for j in range(n):
        ts = [params[j]] + ([grads[j]] if grads is not None else [])
        for t in ts:
            require_device(t)
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != params[j].numel():
                raise BnnHipError(f"{name}: parameters and gradients must be contiguous float32 of one size")
        keep += ts
        a.param[j], a.numel[j] = params[j].data_ptr(), params[j].numel()
        if grads is not None:
            a.grad[j] = grads[j].data_ptr()
    return keep, bank_layout([p.numel() for p in params])[1]


def ivon_draw(params, *, hess: torch.Tensor, ess: float, weight_decay: float, samples: int = 1, sample: int = 0, mean=None,
              step=None, grads=None, acc_g=None, acc_h=None, bank: Optional[torch.Tensor] = None, members: int = 0, first: int = 0,
              sample_base: int = 0, eps_mode: int = L.EPS_PHILOX, seed: int = 0, noise=None):
    """F24 bnn_ivon_draw: theta = m + eps / sqrt(ess (hess + weight_decay)) over lists of fp32 tensors in one launch.
    Training form (`bank` None): draw t * samples + sample (t the device word `step`) into `params`; sample 0 first files the
    parameters (the mean) into `mean`, sample >= 1 reads the mean there and folds `grads` (the previous sample's) into `acc_g`
    / `acc_h`.  Bank form: members first .. first + members - 1 of `bank` ([capacity, stride]) around the mean in `params`,
    member j being draw sample_base + j.  EPS_MEMORY: `noise` [samples, stride] (row `sample`; the fold reads row sample - 1),
    or [members, stride]."""
    lib = L.load()
    S, s, m, first = int(samples), int(sample), int(members), int(first)
    if not 1 <= S <= L.IVON_MAX_SAMPLES or not 0 <= s < S:
        raise BnnHipError(f"ivon_draw: samples must lie in [1, {L.IVON_MAX_SAMPLES}] and sample in [0, samples)")
    if not float(ess) > 0.0 or not float(weight_decay) > 0.0:
        raise BnnHipError("ivon_draw: ess and weight_decay must be > 0")
    a = L.IvonDrawArgs()
    a.struct_bytes = C.sizeof(L.IvonDrawArgs)
    fold = bank is None and s >= 1
    keep, stride = _ivon_tensors("ivon_draw", a, params, grads if fold else None)
    if fold and grads is None:
        raise BnnHipError("ivon_draw: sample >= 1 folds the previous sample's gradients; pass grads, acc_g and acc_h")
    require_device(hess, mean, step, acc_g, acc_h, bank, noise)
    a.samples, a.sample, a.eps_mode = S, s, int(eps_mode)
    a.ess, a.weight_decay, a.seed = float(ess), float(weight_decay), int(seed) & 0xFFFFFFFFFFFFFFFF
    a.hess = _ivon_flat("ivon_draw", "hess", hess, stride)
    if bank is None:
        a.mean = _ivon_flat("ivon_draw", "mean", mean, stride)
        if step is None:
            raise BnnHipError("ivon_draw: the training form needs the step word")
        a.step = _typed(step, torch.int32, "step", 1).data_ptr()
        if fold:
            a.acc_g, a.acc_h = _ivon_flat("ivon_draw", "acc_g", acc_g, stride), _ivon_flat("ivon_draw", "acc_h", acc_h, stride)
        rows = S
    else:
        if not 1 <= m <= L.IVON_MAX_MEMBERS:
            raise BnnHipError(f"ivon_draw: members must lie in [1, {L.IVON_MAX_MEMBERS}], got {m}")
        if bank.dtype != torch.float32 or bank.dim() != 2 or bank.shape[1] != stride or not bank.is_contiguous():
            raise BnnHipError(f"ivon_draw: the bank must be a contiguous float32 [capacity, {stride}] tensor")
        if first < 0 or first + m > bank.shape[0]:
            raise BnnHipError(f"ivon_draw: members [{first}, {first + m}) outside the bank's {bank.shape[0]}")
        a.bank, a.members, a.first, a.capacity = bank.data_ptr(), m, first, bank.shape[0]
        a.sample_base = int(sample_base) & 0xFFFFFFFF
        rows = m
    if eps_mode == L.EPS_MEMORY:
        a.noise = _ivon_flat("ivon_draw", "noise", noise, stride, rows)
    a._keep = keep + [hess, mean, step, acc_g, acc_h, bank, noise]
    L.check(lib.bnn_ivon_draw(C.byref(a), _stream()), "bnn_ivon_draw")


def ivon_step(params, grads, *, lr: float, ess: float, weight_decay: float, beta1: float, beta2: float, loss_scale: float,
              clip_radius: float = float("inf"), samples: int = 1, lr_device=None, mean: torch.Tensor, hess: torch.Tensor,
              avg_grad: torch.Tensor, acc_g=None, acc_h=None, step: torch.Tensor, beta1_prod: torch.Tensor, ticket: torch.Tensor,
              eps_mode: int = L.EPS_PHILOX, seed: int = 0, noise=None):
    """F24 bnn_ivon_step: the variational online Newton step over lists of fp32 tensors in one launch (include/bnn_hip.h F24
    states the chain).  `lr` is the rate used; `step` a one-element int32 device word (read as uint32), `beta1_prod` a
    one-element float64 device word (beta1^step), `ticket` 16 zeroed int32 words; `acc_g` / `acc_h` with samples > 1;
    EPS_MEMORY: `noise` [samples, stride] (the last row is read)."""
    lib = L.load()
    S = int(samples)
    if not 1 <= S <= L.IVON_MAX_SAMPLES:
        raise BnnHipError(f"ivon_step: samples must lie in [1, {L.IVON_MAX_SAMPLES}], got {samples}")
    a = L.IvonStepArgs()
    a.struct_bytes = C.sizeof(L.IvonStepArgs)
    keep, stride = _ivon_tensors("ivon_step", a, params, grads)
    require_device(mean, hess, avg_grad, acc_g, acc_h, step, beta1_prod, ticket, lr_device, noise)
    a.samples, a.eps_mode = S, int(eps_mode)
    a.lr, a.ess, a.weight_decay, a.beta1, a.beta2 = float(lr), float(ess), float(weight_decay), float(beta1), float(beta2)
    a.loss_scale, a.clip_radius, a.lr_device = float(loss_scale), float(clip_radius), _ptr(lr_device)
    a.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    a.mean, a.hess = _ivon_flat("ivon_step", "mean", mean, stride), _ivon_flat("ivon_step", "hess", hess, stride)
    a.avg_grad = _ivon_flat("ivon_step", "avg_grad", avg_grad, stride)
    if S > 1:
        a.acc_g, a.acc_h = _ivon_flat("ivon_step", "acc_g", acc_g, stride), _ivon_flat("ivon_step", "acc_h", acc_h, stride)
    if eps_mode == L.EPS_MEMORY:
        a.noise = _ivon_flat("ivon_step", "noise", noise, stride, S)
    a.step = _typed(step, torch.int32, "step", 1).data_ptr()
    a.beta1_prod = _typed(beta1_prod, torch.float64, "beta1_prod", 1).data_ptr()
    a.ticket = _typed(ticket, torch.int32, "ticket", 16).data_ptr()
    a._keep = keep + [mean, hess, avg_grad, acc_g, acc_h, step, beta1_prod, ticket, lr_device, noise]
    L.check(lib.bnn_ivon_step(C.byref(a), _stream()), "bnn_ivon_step")


# ------------------------------------------------------------------------------------- F23: SVGD / repulsive ensembles
def svgd_chunks(stride: int) -> int:
    """bnn_svgd_chunks: rows of bnn_svgd_dist's partials for a bank of this stride (whole 64-column tiles per chunk, at most
    SVGD_CHUNK columns, about 512 chunks of a smaller bank)."""
    n = int(L.load().bnn_svgd_chunks(int(stride)))
    if n < 1:
        raise BnnHipError(f"svgd_chunks: the stride must be a multiple of 64 in [64, 2^34], got {stride}")
    return n


def _svgd_rows(t: torch.Tensor, members: int, what: str, name: str) -> int:
    """`t` as the first `members` rows of a contiguous float32 [rows, stride] tensor; returns the stride."""
    if not 1 <= members <= L.SVGD_MAX_MEMBERS:
        raise BnnHipError(f"{what}: between 1 and {L.SVGD_MAX_MEMBERS} members, got {members}")
    require_device(t)
    if t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous() or t.shape[0] < members or t.shape[1] < 64 or t.shape[1] % 64:
        raise BnnHipError(f"{what}: {name} must be a contiguous float32 [>= {members}, stride] tensor, stride a multiple of 64, "
                          f"got {tuple(t.shape)} {t.dtype}")
    return int(t.shape[1])


def _svgd_flat(t: torch.Tensor, dtype, numel: int, what: str, name: str) -> torch.Tensor:
    require_device(t)
    if t.dtype != dtype or not t.is_contiguous() or t.numel() < numel:
        raise BnnHipError(f"{what}: {name} must be a contiguous {dtype} tensor of at least {numel} elements")
    return t


def svgd_dist(bank: torch.Tensor, partials: torch.Tensor, *, members: int):
    """F23 bnn_svgd_dist: partials[chunk, pair] = the fp32 sum over the chunk's columns of (bank[i] - bank[j])^2, pair (i, j),
    i < j, at i (2 M - i - 1) / 2 + (j - i - 1); `partials` float32 with svgd_chunks(stride) * M (M - 1) / 2 elements."""
    lib = L.load()
    M = int(members)
    stride = _svgd_rows(bank, M, "svgd_dist", "bank")
    _svgd_flat(partials, torch.float32, max(1, svgd_chunks(stride) * (M * (M - 1) // 2)), "svgd_dist", "partials")
    a = L.SvgdDistArgs()
    a.struct_bytes = C.sizeof(L.SvgdDistArgs)
    a.members, a.stride, a.bank, a.partials = M, stride, bank.data_ptr(), partials.data_ptr()
    a._keep = (bank, partials)
    L.check(lib.bnn_svgd_dist(C.byref(a), _stream()), "bnn_svgd_dist")
    return partials


def svgd_coef(partials: torch.Tensor, coef: torch.Tensor, record: torch.Tensor, *, members: int, chunks: int, grad_scale: float,
              tau: float, method: int = L.SVGD_SVGD, bandwidth: float = 0.0):
    """F23 bnn_svgd_coef: the chunk partials -> D2, its median, h (bandwidth 0: median / log(M + 1)), K, r and coef = [A | B]
    (float32 [M, 2 M]); `record` float64 [svgd_record_doubles(M)]: D2, med, h, r."""
    lib = L.load()
    M, chunks = int(members), int(chunks)
    if not 1 <= M <= L.SVGD_MAX_MEMBERS or chunks < 1:
        raise BnnHipError(f"svgd_coef: between 1 and {L.SVGD_MAX_MEMBERS} members and chunks >= 1 are required")
    _svgd_flat(partials, torch.float32, max(1, chunks * (M * (M - 1) // 2)), "svgd_coef", "partials")
    _svgd_flat(coef, torch.float32, 2 * M * M, "svgd_coef", "coef")
    _svgd_flat(record, torch.float64, L.svgd_record_doubles(M), "svgd_coef", "record")
    a = L.SvgdCoefArgs()
    a.struct_bytes = C.sizeof(L.SvgdCoefArgs)
    a.members, a.chunks, a.method = M, chunks, int(method)
    a.grad_scale, a.tau, a.bandwidth = float(grad_scale), float(tau), float(bandwidth)
    a.partials, a.coef, a.record = partials.data_ptr(), coef.data_ptr(), record.data_ptr()
    a._keep = (partials, coef, record)
    L.check(lib.bnn_svgd_coef(C.byref(a), _stream()), "bnn_svgd_coef")
    return coef, record


def svgd_direction(coef: torch.Tensor, bank: torch.Tensor, bucket: torch.Tensor, *, members: int):
    """F23 bnn_svgd_direction: bucket[:M] <- coef . [bucket[:M] ; bank[:M]] per column, in place (coef float32 [M, 2 M])."""
    lib = L.load()
    M = int(members)
    stride = _svgd_rows(bank, M, "svgd_direction", "bank")
    if _svgd_rows(bucket, M, "svgd_direction", "bucket") != stride:
        raise BnnHipError("svgd_direction: the bucket must have the bank's stride")
    _svgd_flat(coef, torch.float32, 2 * M * M, "svgd_direction", "coef")
    a = L.SvgdDirectionArgs()
    a.struct_bytes = C.sizeof(L.SvgdDirectionArgs)
    a.members, a.stride = M, stride
    a.coef, a.bank, a.bucket = coef.data_ptr(), bank.data_ptr(), bucket.data_ptr()
    a._keep = (coef, bank, bucket)
    L.check(lib.bnn_svgd_direction(C.byref(a), _stream()), "bnn_svgd_direction")
    return bucket


def bank_fwd(x: torch.Tensor, bank: torch.Tensor, w_off: int, b_off: Optional[int], *, out_features: int, members: int,
             first: int = 0, relu: bool = False, math_mode: int = L.MATH_F32, y_dtype=torch.float32, out=None) -> torch.Tensor:
    """F19 bnn_bank_fwd: y[j] = act(x[j or shared] . W[first + j]^T + b[first + j]) for `members` members of `bank` (float32
    [capacity, stride]) in one launch; member m's [out, in] weights start at bank[m, w_off], its bias at bank[m, b_off] (None:
    no bias).  x [B, in] (shared) or [members, B, in]; returns [members, B, out] of y_dtype.  Bit-equal per member to
    dense_fwd(x_j, W_m, b_m, n_samples=1, drop_p=0)."""
    lib = L.load()
    require_device(x, bank, out)
    M, first, N = int(members), int(first), int(out_features)
    if bank.dtype != torch.float32 or bank.dim() != 2 or not bank.is_contiguous():
        raise BnnHipError("bank_fwd: the bank must be a contiguous float32 [capacity, stride] tensor")
    if M < 1 or first < 0 or first + M > bank.shape[0]:
        raise BnnHipError(f"bank_fwd: members [{first}, {first + M}) lie outside the bank's {bank.shape[0]} slots")
    if x.dim() == 2:
        shared, B, K = 1, x.shape[0], x.shape[1]
    elif x.dim() == 3 and x.shape[0] == M:
        shared, B, K = 0, x.shape[1], x.shape[2]
    else:
        raise BnnHipError(f"bank_fwd: x must be [batch, in] or [{M}, batch, in], got {tuple(x.shape)}")
    stride = bank.shape[1]
    if N < 1 or w_off < 0 or w_off + N * K > stride or (b_off is not None and (b_off < 0 or b_off + N > stride)):
        raise BnnHipError("bank_fwd: the layer's weights / bias lie outside a member")
    x = x if x.is_contiguous() else x.contiguous()
    if out is None:
        out = torch.empty((M, B, N), dtype=y_dtype, device=x.device)
    elif tuple(out.shape) != (M, B, N) or not out.is_contiguous():
        raise BnnHipError(f"bank_fwd: out must be a contiguous [{M}, {B}, {N}] tensor")
    a = L.BankFwdArgs()
    a.struct_bytes = C.sizeof(L.BankFwdArgs)
    a.members, a.first, a.batch, a.in_features, a.out_features = M, first, B, K, N
    a.x_shared, a.relu, a.x, a.x_dtype, a.math = shared, int(bool(relu)), x.data_ptr(), _dt(x), int(math_mode)
    a.w, a.w_stride = bank.data_ptr() + 4 * int(w_off), stride
    if b_off is not None:
        a.b, a.b_stride = bank.data_ptr() + 4 * int(b_off), stride
    a.y, a.y_dtype = out.data_ptr(), _dt(out)
    a._keep = (x, bank, out)
    L.check(lib.bnn_bank_fwd(C.byref(a), _stream()), "bnn_bank_fwd")
    return out


# ------------------------------------------------------------------------------------- F21: training a deep ensemble
def _ens_bank(bank: torch.Tensor, members: int, first: int, what: str) -> int:
    """Checks `bank` (float32 [capacity, stride], contiguous, on the device) and the member span; returns the stride."""
    require_device(bank)
    if bank.dtype != torch.float32 or bank.dim() != 2 or not bank.is_contiguous():
        raise BnnHipError(f"{what}: the bank must be a contiguous float32 [capacity, stride] tensor")
    if members < 1 or first < 0 or first + members > bank.shape[0]:
        raise BnnHipError(f"{what}: members [{first}, {first + members}) lie outside the bank's {bank.shape[0]} slots")
    return int(bank.shape[1])


def _ens_act(t: Optional[torch.Tensor], shape: tuple, what: str):
    if t is not None and (tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous()):
        raise BnnHipError(f"{what}: expected a contiguous float32 tensor of shape {shape}, got {tuple(t.shape)} {t.dtype}")


def ens_fwd(x: torch.Tensor, bank: torch.Tensor, w_off: int, b_off: Optional[int], *, out_features: int, members: int,
            first: int = 0, relu: bool = False, drop_p: float = 0.0, layer_id: int = 0, seed: int = 0, sample_offset: int = 0,
            sample_counter=None, sample_counter_inc: int = 0, math_mode: int = L.MATH_F32, out=None) -> torch.Tensor:
    """F21 bnn_ens_fwd: y[j] = drop_j(act(x[j or shared] . W[first + j]^T + b[first + j])) for `members` members of `bank` in one
    launch, fp32 in and out; the kind-3 mask of `layer_id` at global sample index sample_offset + *sample_counter + j.  x
    [B, in] (shared) or [members, B, in]; returns [members, B, out].  Bit-equal per member to dense_fwd(x_j, W, b, n_samples=1)
    at that index."""
    lib = L.load()
    M, first, N = int(members), int(first), int(out_features)
    stride = _ens_bank(bank, M, first, "ens_fwd")
    require_device(x, out, sample_counter)
    dropout_params(drop_p)
    if x.dim() == 2:
        shared, B, K = 1, x.shape[0], x.shape[1]
    elif x.dim() == 3 and x.shape[0] == M:
        shared, B, K = 0, x.shape[1], x.shape[2]
    else:
        raise BnnHipError(f"ens_fwd: x must be [batch, in] or [{M}, batch, in], got {tuple(x.shape)}")
    _ens_act(x, tuple(x.shape), "ens_fwd")
    if N < 1 or w_off < 0 or w_off + N * K > stride or (b_off is not None and (b_off < 0 or b_off + N > stride)):
        raise BnnHipError("ens_fwd: the layer's weights / bias lie outside a member")
    if out is None:
        out = torch.empty((M, B, N), dtype=torch.float32, device=x.device)
    _ens_act(out, (M, B, N), "ens_fwd")
    if sample_counter is not None and (sample_counter.dtype != torch.int32 or sample_counter.numel() != 1):
        raise BnnHipError("ens_fwd: sample_counter must be a one-element int32 device tensor")
    a = L.EnsFwdArgs()
    a.struct_bytes = C.sizeof(L.EnsFwdArgs)
    a.members, a.first, a.batch, a.in_features, a.out_features = M, first, B, K, N
    a.x_shared, a.relu, a.math, a.layer_id = shared, int(bool(relu)), _exact_unless_bf16(int(math_mode)), int(layer_id)
    a.x, a.w, a.w_stride = x.data_ptr(), bank.data_ptr() + 4 * int(w_off), stride
    if b_off is not None:
        a.b, a.b_stride = bank.data_ptr() + 4 * int(b_off), stride
    a.drop_p, a.seed, a.sample_offset = float(drop_p), int(seed) & 0xFFFFFFFFFFFFFFFF, int(sample_offset) & 0xFFFFFFFF
    a.sample_counter, a.sample_counter_inc = _ptr(sample_counter), int(sample_counter_inc)
    a.y = out.data_ptr()
    a._keep = (x, bank, out, sample_counter)
    L.check(lib.bnn_ens_fwd(C.byref(a), _stream()), "bnn_ens_fwd")
    return out


def ens_loss(logits: torch.Tensor, target: torch.Tensor, mode: str, *, grad_scale: float = 1.0, loss=None, g_logits=None):
    """F21 bnn_ens_loss: (loss [M], g_logits [M, B, C]) of dense_loss per member of logits [M, B, C], one launch.  target:
    one for all members (int64 [B] / float32 of B * C elements) or one per member (M times as many elements)."""
    lib = L.load()
    require_device(logits, target, loss, g_logits)
    if logits.dim() != 3:
        raise BnnHipError(f"ens_loss: logits must be [members, batch, classes], got {tuple(logits.shape)}")
    _ens_act(logits, tuple(logits.shape), "ens_loss")
    M, B, Cc = logits.shape
    if mode == "classification":
        lm, per, dt = L.NLL_CLASSIFICATION, B, torch.int64
    elif mode == "regression":
        lm, per, dt = L.NLL_REGRESSION, B * Cc, torch.float32
    else:
        raise BnnHipError(f"ens_loss: unknown mode {mode!r}")
    if target.dtype != dt or target.numel() not in (per, M * per) or not target.is_contiguous():
        raise BnnHipError(f"ens_loss: {mode} targets must be contiguous {dt} with {per} (shared) or {M * per} elements")
    shared = int(target.numel() == per)
    if loss is None:
        loss = torch.empty((M,), dtype=torch.float32, device=logits.device)
    _ens_act(loss, (M,), "ens_loss")
    if g_logits is None:
        g_logits = torch.empty_like(logits)
    _ens_act(g_logits, (M, B, Cc), "ens_loss")
    a = L.EnsLossArgs()
    a.struct_bytes = C.sizeof(L.EnsLossArgs)
    a.members, a.batch, a.classes, a.loss_mode, a.target_shared = M, B, Cc, lm, shared
    a.grad_scale = float(grad_scale)
    a.logits, a.target, a.loss, a.g_logits = logits.data_ptr(), target.data_ptr(), loss.data_ptr(), g_logits.data_ptr()
    L.check(lib.bnn_ens_loss(C.byref(a), _stream()), "bnn_ens_loss")
    return loss, g_logits


def ens_bwd(x: torch.Tensor, gy: torch.Tensor, bank: torch.Tensor, w_off: int, bucket: torch.Tensor, b_off: Optional[int] = None,
            *, first: int = 0, g_x=None, y=None, y_scale: float = 1.0, gx_mask: bool = False, gx_scale: float = 1.0,
            math_mode: int = L.MATH_F32):
    """F21 bnn_ens_bwd: dense_bwd for every member in one launch.  gy [M, B, out]; x [B, in] (shared) or [M, B, in]; member
    first + j's weights at bank[first + j, w_off]; its gradients go to bucket[j, w_off] ([out, in]) and bucket[j, b_off]
    ([out]; None: no bias gradient), `bucket` float32 [M, stride] in the bank's layout; g_x (optional) [M, B, in]."""
    lib = L.load()
    if gy.dim() != 3:
        raise BnnHipError(f"ens_bwd: gy must be [members, batch, out], got {tuple(gy.shape)}")
    M, B, N = gy.shape
    first = int(first)
    stride = _ens_bank(bank, M, first, "ens_bwd")
    require_device(x, gy, bucket, g_x, y)
    if x.dim() == 2 and x.shape[0] == B:
        shared, K = 1, x.shape[1]
    elif x.dim() == 3 and x.shape[0] == M and x.shape[1] == B:
        shared, K = 0, x.shape[2]
    else:
        raise BnnHipError(f"ens_bwd: x must be [{B}, in] or [{M}, {B}, in], got {tuple(x.shape)}")
    for t, shp in ((x, tuple(x.shape)), (gy, (M, B, N)), (y, (M, B, N)), (g_x, (M, B, K)), (bucket, (M, stride))):
        _ens_act(t, shp, "ens_bwd")
    if w_off < 0 or w_off + N * K > stride or (b_off is not None and (b_off < 0 or b_off + N > stride)):
        raise BnnHipError("ens_bwd: the layer's weights / bias lie outside a member")
    a = L.EnsBwdArgs()
    a.struct_bytes = C.sizeof(L.EnsBwdArgs)
    a.members, a.first, a.batch, a.in_features, a.out_features = M, first, B, K, N
    a.x_shared, a.math, a.gx_mask = shared, _exact_unless_bf16(int(math_mode)), int(bool(gx_mask))
    a.y_scale, a.gx_scale = float(y_scale), float(gx_scale)
    a.x, a.gy, a.y = x.data_ptr(), gy.data_ptr(), _ptr(y)
    a.w, a.w_stride, a.g_stride = bank.data_ptr() + 4 * int(w_off), stride, stride
    a.g_w = bucket.data_ptr() + 4 * int(w_off)
    if b_off is not None:
        a.g_b = bucket.data_ptr() + 4 * int(b_off)
    a.g_x = _ptr(g_x)
    a._keep = (x, gy, y, bank, bucket, g_x)
    L.check(lib.bnn_ens_bwd(C.byref(a), _stream()), "bnn_ens_bwd")


# ------------------------------------------------------------------------------------- F20: Kronecker-factored Laplace
def _kfac_rows(x, gy, w, what: str):
    """(B, R, in, out) of a layer call's x [B, in], gy [R, out], w [out, in]."""
    x = _lap_f32(x, "x")
    if x.dim() != 2:
        raise BnnHipError(f"{what}: x must be [batch, in], got {tuple(x.shape)}")
    B, K = x.shape
    N = w.shape[0]
    gy = _lap_f32(gy, "gy")
    if gy.dim() != 2 or gy.shape[0] % B != 0:
        raise BnnHipError(f"{what}: gy must be [rows, out] with rows a multiple of the batch {B}, got {tuple(gy.shape)}")
    R = gy.shape[0]
    _lap_f32(gy, "gy", (R, N)), _lap_f32(w, "w", (N, K))
    return B, R, K, N


def kfac_layer(x, gy, w, *, a, s, g, g_x=None, y=None, gx_mask: bool = False, math_mode: int = L.MATH_F32):
    """F20 bnn_kfac_layer: one Linear -> [ReLU] group.  x [B, in], gy [R, out] (R a multiple of B), the saved output
    y [B, out] (gz = y > 0 ? gy : 0) or None; a [in, in] += x^T x, s [in] += colsum(x), g [out, out] += gz^T gz (exact fp32,
    bit-symmetric); g_x [R, in] = gz w as laplace_layer's (the same bits)."""
    lib = L.load()
    B, R, K, N = _kfac_rows(x, gy, w, "kfac_layer")
    if a is None or s is None or g is None:
        raise BnnHipError("kfac_layer: the factors (a, s, g) are needed")
    _lap_f32(a, "a", (K, K)), _lap_f32(s, "s", (K,)), _lap_f32(g, "g", (N, N))
    _lap_f32(g_x, "g_x", (R, K)), _lap_f32(y, "y", (B, N))
    k = L.KfacLayerArgs()
    k.struct_bytes = C.sizeof(L.KfacLayerArgs)
    k.batch, k.rows, k.in_features, k.out_features = B, R, K, N
    k.math, k.gx_mask = _exact_unless_bf16(math_mode), int(bool(gx_mask))
    k.x, k.gy, k.y, k.w = x.data_ptr(), gy.data_ptr(), _ptr(y), w.data_ptr()
    k.a, k.s, k.g, k.g_x = a.data_ptr(), s.data_ptr(), g.data_ptr(), _ptr(g_x)
    L.check(lib.bnn_kfac_layer(C.byref(k), _stream()), "bnn_kfac_layer")


def kfac_evidence(weights, biases, lambdas_a, lambdas_g, precisions, *, record, log_evidence=None, best_index=None, best=None,
                  workspace=None):
    """F20 bnn_kfac_evidence: the Laplace log marginal likelihood in the Kronecker eigenbasis at every candidate prior precision
    (host floats) -> (log_evidence float64 [G], best_index int32 [1], best float64 [2] = (maximum, its precision)).  Per layer
    the weight [out, in], the bias [out] and the float64 eigenvalues lambda_a [in + 1], lambda_g [out].  Nothing is read back."""
    lib = L.load()
    taus = [float(t) for t in precisions]
    G, n = len(taus), len(weights)
    if not 1 <= G <= L.LAPLACE_MAX_PRECISIONS:
        raise BnnHipError(f"kfac_evidence: between 1 and {L.LAPLACE_MAX_PRECISIONS} candidate precisions, got {G}")
    if not all(0.0 < t < math.inf for t in taus):
        raise BnnHipError("kfac_evidence: prior precisions must be positive and finite")
    if not 1 <= n <= L.LAPLACE_GLM_MAX_LAYERS or not len(biases) == len(lambdas_a) == len(lambdas_g) == n:
        raise BnnHipError(f"kfac_evidence: between 1 and {L.LAPLACE_GLM_MAX_LAYERS} layers, each with weight, bias and two eigenvalue vectors")
    a = L.KfacEvidenceArgs()
    a.struct_bytes = C.sizeof(L.KfacEvidenceArgs)
    a.n_layers, a.n_precisions = n, G
    for l, (w, b, la, lg) in enumerate(zip(weights, biases, lambdas_a, lambdas_g)):
        _lap_f32(w, "weight")
        N, K = w.shape
        _lap_f32(b, "bias", (N,)), _lap_f64(la, "lambda_a", K + 1), _lap_f64(lg, "lambda_g", N)
        a.weight[l], a.bias[l], a.lambda_a[l], a.lambda_g[l] = w.data_ptr(), b.data_ptr(), la.data_ptr(), lg.data_ptr()
        a.in_features[l], a.out_features[l] = K, N
    for g, t in enumerate(taus):
        a.precision[g] = t
    dev = weights[0].device
    need = lib.bnn_kfac_evidence_workspace_bytes(C.byref(a))
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty(need // 8, dtype=torch.float64, device=dev)
    log_evidence = torch.empty(G, dtype=torch.float64, device=dev) if log_evidence is None else _lap_f64(log_evidence, "log_evidence", G)
    best_index = torch.zeros(1, dtype=torch.int32, device=dev) if best_index is None else _typed(best_index, torch.int32, "best_index", 1)
    best = torch.zeros(2, dtype=torch.float64, device=dev) if best is None else _lap_f64(best, "best", 2)
    a.record = _lap_f64(record, "record", L.LAPLACE_RECORD_DOUBLES).data_ptr()
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    a.log_evidence, a.best_index, a.best = log_evidence.data_ptr(), best_index.data_ptr(), best.data_ptr()
    L.check(lib.bnn_kfac_evidence(C.byref(a), _stream()), "bnn_kfac_evidence")
    return log_evidence, best_index, best


def kfac_glm_rotate(x, gy, w, *, q_a, q_g, at=None, gt=None, g_x=None, y=None, gx_mask: bool = False, math_mode: int = L.MATH_F32):
    """F20 bnn_kfac_glm_rotate: at [B, in + 1] = [x | 1] q_a, gt [R, out] = gz q_g (exact fp32; eigenvectors in columns) and
    g_x [R, in] = gz w as laplace_layer's, in one launch.  Returns (at, gt)."""
    lib = L.load()
    B, R, K, N = _kfac_rows(x, gy, w, "kfac_glm_rotate")
    glm_pairs(R // B)
    if q_a is None or q_g is None:
        raise BnnHipError("kfac_glm_rotate: the eigenvectors (q_a, q_g) are needed")
    _lap_f32(q_a, "q_a", (K + 1, K + 1)), _lap_f32(q_g, "q_g", (N, N)), _lap_f32(g_x, "g_x", (R, K)), _lap_f32(y, "y", (B, N))
    at = torch.empty((B, K + 1), dtype=torch.float32, device=x.device) if at is None else _lap_f32(at, "at", (B, K + 1))
    gt = torch.empty((R, N), dtype=torch.float32, device=x.device) if gt is None else _lap_f32(gt, "gt", (R, N))
    a = L.KfacGlmRotateArgs()
    a.struct_bytes = C.sizeof(L.KfacGlmRotateArgs)
    a.batch, a.rows, a.in_features, a.out_features = B, R, K, N
    a.math, a.gx_mask = _exact_unless_bf16(math_mode), int(bool(gx_mask))
    a.x, a.gy, a.y, a.w = x.data_ptr(), gy.data_ptr(), _ptr(y), w.data_ptr()
    a.q_a, a.q_g, a.at, a.gt, a.g_x = q_a.data_ptr(), q_g.data_ptr(), at.data_ptr(), gt.data_ptr(), _ptr(g_x)
    L.check(lib.bnn_kfac_glm_rotate(C.byref(a), _stream()), "bnn_kfac_glm_rotate")
    return at, gt


def kfac_glm_var(at, gt, lambda_a, lambda_g, *, cov_part=None, v_out=None, precision=None, precision_device=None):
    """F20 bnn_kfac_glm_var: V [B, out] = at^2 . D^T with D_ji = 1 / (lambda_g[j] lambda_a[i] + tau) formed while staging, and
    the tile partials of sum_j gt_c gt_c' V into cov_part [ceil(out / 64), B, C (C + 1) / 2] (laplace_glm_finish's layout).
    at [B, in + 1], gt [B * C, out] float32; the eigenvalues float64; tau a host float or a one-element float64 device tensor."""
    lib = L.load()
    at, gt = _lap_f32(at, "at"), _lap_f32(gt, "gt")
    if at.dim() != 2 or gt.dim() != 2 or at.shape[1] < 2 or gt.shape[0] % at.shape[0] != 0:
        raise BnnHipError(f"kfac_glm_var: at must be [batch, in + 1] and gt [batch * C, out], got {tuple(at.shape)}, {tuple(gt.shape)}")
    B, K1 = at.shape
    R, N = gt.shape
    P = glm_pairs(R // B)
    _lap_f64(lambda_a, "lambda_a", K1), _lap_f64(lambda_g, "lambda_g", N), _lap_f32(v_out, "v_out", (B, N))
    shape = (glm_tiles(N), B, P)
    cov_part = torch.empty(shape, dtype=torch.float32, device=at.device) if cov_part is None else _lap_f32(cov_part, "cov_part", shape)
    a = L.KfacGlmVarArgs()
    a.struct_bytes = C.sizeof(L.KfacGlmVarArgs)
    a.batch, a.rows, a.in_features, a.out_features = B, R, K1 - 1, N
    _glm_precision(a, precision, precision_device, "kfac_glm_var")
    a.at, a.gt, a.lambda_a, a.lambda_g = at.data_ptr(), gt.data_ptr(), lambda_a.data_ptr(), lambda_g.data_ptr()
    a.cov_part, a.v_out = cov_part.data_ptr(), _ptr(v_out)
    L.check(lib.bnn_kfac_glm_var(C.byref(a), _stream()), "bnn_kfac_glm_var")
    return cov_part


def kfac_sample(w, b, q_a, q_g, lambda_a, lambda_g, bank: torch.Tensor, w_off: int, b_off: int, *, members: int, first: int = 0,
                layer: int, seed: int, sample_base: int = 0, precision=None, precision_device=None, workspace=None):
    """F20 bnn_kfac_sample: `members` matrix-normal draws Wbar + q_g (E o Sigma) q_a^T of one layer into slots first ... of
    `bank` (float32 [capacity, stride]; the weight at bank[m, w_off], the bias at bank[m, b_off]), two launches.  The noise of
    draw m is the Philox stream (e >> 2, sample_base + m, layer, 4), slot e & 3.  Returns the workspace (reusable)."""
    lib = L.load()
    require_device(bank, workspace)
    _lap_f32(w, "w")
    N, K = w.shape
    _lap_f32(b, "b", (N,)), _lap_f32(q_a, "q_a", (K + 1, K + 1)), _lap_f32(q_g, "q_g", (N, N))
    _lap_f64(lambda_a, "lambda_a", K + 1), _lap_f64(lambda_g, "lambda_g", N)
    M, first = int(members), int(first)
    if bank.dtype != torch.float32 or bank.dim() != 2 or not bank.is_contiguous():
        raise BnnHipError("kfac_sample: the bank must be a contiguous float32 [capacity, stride] tensor")
    if M < 1 or first < 0 or first + M > bank.shape[0]:
        raise BnnHipError(f"kfac_sample: members [{first}, {first + M}) lie outside the bank's {bank.shape[0]} slots")
    stride = bank.shape[1]
    if w_off < 0 or w_off + N * K > stride or b_off < 0 or b_off + N > stride:
        raise BnnHipError("kfac_sample: the layer's weights / bias lie outside a member")
    need = lib.bnn_kfac_sample_workspace_bytes(M, K, N)
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty(need // 4, dtype=torch.float32, device=bank.device)
    a = L.KfacSampleArgs()
    a.struct_bytes = C.sizeof(L.KfacSampleArgs)
    a.members, a.first, a.in_features, a.out_features = M, first, K, N
    a.layer, a.sample_base, a.seed = int(layer) & 0xFFFFFFFF, int(sample_base) & 0xFFFFFFFF, int(seed) & 0xFFFFFFFFFFFFFFFF
    _glm_precision(a, precision, precision_device, "kfac_sample")
    a.w, a.b, a.q_a, a.q_g = w.data_ptr(), b.data_ptr(), q_a.data_ptr(), q_g.data_ptr()
    a.lambda_a, a.lambda_g = lambda_a.data_ptr(), lambda_g.data_ptr()
    a.bank, a.bank_stride, a.w_offset, a.b_offset = bank.data_ptr(), stride, int(w_off), int(b_off)
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    L.check(lib.bnn_kfac_sample(C.byref(a), _stream()), "bnn_kfac_sample")
    return workspace
