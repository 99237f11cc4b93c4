"""TEST INFRASTRUCTURE: fp64 restatement of the dense layer -- K5 bnn_dense_fwd (csrc/mlp_dropout.hip) and K6 bnn_dense_bwd
(csrc/dense_train.hip on the tile core of csrc/dense_tile.h) -- at the kernels' rounding points, with a bound for EVERY
output element, the one table of cases both test files walk, and the seeded wrong variants the bound has to reject.
torch-CPU and numpy only: imports without a GPU.  tests/test_dense_layer_cpu.py proves the restatement and the bound;
tests/test_gpu_dense_layer.py holds the kernels to them.

What is restated
----------------
Forward.   y[s] = drop_s(act(x[s or shared] W^T + b)): the kind-3 mask of tests/test_mc_dropout_cpu.dropout_mask_np at the
           global sample index (sample_offset + counter + s) mod 2^32, times the fp32 scale of ops.dropout_params.  bf16
           math rounds x and W to bf16 (RNE) before the product -- their products are exact in fp32 and the accumulation
           is fp32, so the sum stays in fp64 here -- and the result is rounded to bf16 only when y is bf16.
Backward.  gz = gy (y None) or (y > 0 ? fl32(gy * y_scale) : 0): ONE fp32 product, restated as an fp32 product.
           g_w = gz^T x, g_b = colsum(gz), g_x = gz W [* (x > 0 ? gx_scale : 0)].  bf16 math changes g_x alone: its
           operands are bf16(gz) and bf16(W), exactly representable, so that sum stays in fp64 too.
y, x and the masks are INPUTS: no element is ever excluded for a mask reason.

The bound
---------
The model and the constants are tests/layer_bwd_ref.py's (U = 2^-24, C_TAIL = 16; Higham 3.1 to first order, ANY summation
order, which is why the MFMA tile order, the 32-wide stages and g_b's four partial sums do not matter):

    |got - ref| <= (n + C_TAIL) * U * sum_i |t_i|,      sum |t_i| the same formula on absolute values, in fp64,

with n the reduction length: `in` for the forward (|b| one more term of the sum), `out` for g_x, `batch` for g_w and g_b.
The elementwise tail C_TAIL covers holds at most TWO roundings here: the forward's bias add and its product with the mask
scale (ReLU is exact and 1-Lipschitz, so the bound of z carries over to relu(z) with no exclusion around zero); g_x's
product with gx_scale; nothing for g_w and g_b.  gz's product is restated exactly and costs nothing.  A dropped element
(mask 0, x <= 0 under gx_mask) has bound 0: it has to be exactly 0.
bf16 output: the fp32 value the kernel rounds lies in [lo, hi] = [ref - bound, ref + bound] (under ReLU the ends are those
of the pre-activation, passed through ReLU and the mask, which are monotone: a value that is negative by more than its
bound gives [0, 0]); rounding is monotone, so `got` has to lie in [bf16(lo), bf16(hi)] -- layer_bwd_ref.bf16_tie's rule.
`info["tie_share"]` is the share of elements whose two ends differ (the interval straddles a rounding tie and either
neighbour is legitimate); it is a CONDITION on the table, below 1 % for every case from the reference alone
(tests/test_dense_layer_cpu.py), which is why the bf16-y cases have reductions of at most 32.
Nothing here was fitted to what a kernel produced.
"""
import collections
import functools
import zlib

import numpy as np
import torch

from layer_bwd_ref import C_TAIL, U, bf16_tie, bf16r
from test_mc_dropout_cpu import dropout_mask_np

F64 = torch.float64
F32 = torch.float32
SEED, LAYER_ID = 0x0F1E2D3C4B5A6978, 2
WRAP = 2 ** 32 - 2
TILE, STAGE = 64, 32
MIN_BLOCKS, MIN_SAMPLES_PER_RUN = 512, 4        # csrc/mlp_dropout.hip: kMinBlocks, kMinSamplesPerRun

Fwd = collections.namedtuple("Fwd", "y bound lo hi info")
Bwd = collections.namedtuple("Bwd", "grads bounds")             # (g_w, g_b, g_x); None where the case does not ask for one
BWD_NAMES = ("g_w", "g_b", "g_x")


# ------------------------------------------------------------------------------------------------------------ pieces
def bf16_trunc(t):
    """fp32 -> bf16 by truncation (the seeded wrong rounding)."""
    bits = t.to(F32).contiguous().view(torch.int32) & -65536
    return bits.view(F32).to(t.dtype)


def mm_exact(a, b):
    """sum_k a[..., m, k] b[n, k] in the tensors' own dtype and torch's order."""
    return a @ b.transpose(-1, -2)


def mm_seq(a, b):
    """The same sum, one k after the other: acc = fl(acc + fl(a b))."""
    acc = torch.zeros(a.shape[:-1] + (b.shape[0],), dtype=a.dtype)
    for k in range(a.shape[-1]):
        acc = acc + a[..., k:k + 1] * b[:, k]
    return acc


def mm_staged(width):
    """The kernels' walk: blocks of `width` k (32: one bf16 MFMA; 4: one fp32 MFMA) summed from zero, then added to the
    accumulator in k order."""
    def mm(a, b):
        acc = torch.zeros(a.shape[:-1] + (b.shape[0],), dtype=a.dtype)
        for k0 in range(0, a.shape[-1], width):
            acc = acc + mm_seq(a[..., k0:k0 + width], b[:, k0:k0 + width])
        return acc
    return mm


def plan_runs(rows, out, S, shared):
    """The sample runs of a shared-x launch (dense_check in csrc/mlp_dropout.hip) at the 64 x 64 tile: (runs, per)."""
    if not shared:
        return 1, S
    tiles = -(-rows // TILE) * -(-out // TILE)
    runs = max(1, min(-(-MIN_BLOCKS // tiles), -(-S // MIN_SAMPLES_PER_RUN)))
    per = -(-S // runs)
    return -(-S // per), per


def masks(S, B, N, p, sample0, variant=None):
    """float64 [S, B, N]: the launch's masks (scale where kept, 0 where dropped), or a seeded wrong one."""
    if p == 0.0:
        return torch.ones(S, B, N, dtype=F64)
    out = []
    for s in range(S):
        g = (sample0 + s + (1 if variant == "mask_shift_sample" else 0)) & 0xFFFFFFFF
        if variant == "mask_shift_col":                           # the group of the next four columns (row-major)
            gpr = (N + 3) // 4
            m = dropout_mask_np(SEED, LAYER_ID, g, B, 4 * gpr, p).reshape(B * gpr, 4)
            m = np.roll(m, -1, axis=0).reshape(B, 4 * gpr)[:, :N]
        else:
            m = dropout_mask_np(SEED, LAYER_ID, g, B, N, p)
        out.append(torch.from_numpy(np.ascontiguousarray(m)).to(F64))
    return torch.stack(out)


# ------------------------------------------------------------------------------------------------------------ forward
def fwd_ref(x, w, b, *, S, relu, drop_p, sample0, bf16, y_bf16, dtype=F64, mm=mm_exact, variant=None, want_bound=True):
    """y [S, B, N] of one bnn_dense_fwd launch, its bound and, for a bf16 y, the two ends `got` has to lie between.
    x [B, K] (shared) or [S, B, K], fp32 or bf16.  dtype / mm: the arithmetic of the evaluation (fp64 exact: the reference).
    A seeded variant and an fp32 evaluation round a bf16 y as the kernel would; the reference itself stays unrounded."""
    dt = dtype
    shared = x.dim() == 2
    B, K = x.shape[-2], x.shape[-1]
    N = w.shape[0]
    rnd = bf16_trunc if variant == "bf16_trunc" else bf16r
    xs, ws = x.to(dt).clone(), w.to(dt)
    bs = None if b is None else b.to(dt).clone()
    if bf16:
        xs, ws = rnd(xs), rnd(ws)
    ax, aw = xs.abs(), ws.abs()
    if variant == "drop_last_k":
        xs[..., -1] = 0
    elif variant == "tail_from_8":
        xs[..., (K // 8) * 8:] = 0
    elif variant == "row64_from_63":
        flat = xs.view(-1, K)
        flat[64] = flat[63]
    elif variant == "bias_last_group":
        bs[(N // 4) * 4:] = 0
    z = mm(xs, ws)
    if bs is not None:
        z = z + bs
    zpre = z
    if relu:
        z = torch.relu(z)
    m = masks(S, B, N, drop_p, sample0, variant).to(dt)
    y = (z if not shared else z.unsqueeze(0)) * m
    if variant == "skip_last_run":
        runs, per = plan_runs(B, N, S, shared)
        y[(runs - 1) * per:] = 0
    if y_bf16 and (variant is not None or dt != F64):
        y = rnd(y)
    if not want_bound:
        return Fwd(y, None, None, None, {})
    A = mm_exact(ax, aw)
    if b is not None:
        A = A + b.to(dt).abs()
    bz = (K + C_TAIL) * U * A
    bound = (bz if not shared else bz.unsqueeze(0)) * m
    lo, hi, info = None, None, {"tie_share": 0.0}
    if y_bf16:
        lo, hi = zpre - bz, zpre + bz
        if relu:
            lo, hi = torch.relu(lo), torch.relu(hi)
        lo, hi = (lo if not shared else lo.unsqueeze(0)) * m, (hi if not shared else hi.unsqueeze(0)) * m
        _, slack = bf16_tie((lo + hi) / 2, (hi - lo) / 2)
        info["tie_share"] = float((slack > 0).double().mean())
        lo, hi = bf16r(lo), bf16r(hi)
    return Fwd(y, bound, lo, hi, info)


# ------------------------------------------------------------------------------------------------------------ backward
def bwd_ref(x, gy, w, y, *, y_scale, gx_mask, gx_scale, bf16, want_gb=True, want_gx=True, dtype=F64, mm=mm_exact,
            variant=None, want_bound=True):
    """(g_w [N, K], g_b [N], g_x [B, K]) of one bnn_dense_bwd launch and their bounds.  x [B, K], gy / y [B, N], w [N, K]."""
    dt = dtype
    B, K = x.shape
    N = w.shape[0]
    rnd = bf16_trunc if variant == "bf16_trunc" else bf16r
    xs, ws = x.to(dt), w.to(dt)
    if y is None:
        gz = gy.to(dt)
    else:
        live = (y >= 0) if variant == "y_ge" else (y > 0)
        prod = gy.to(F32) if variant == "no_y_scale" else gy.to(F32) * torch.tensor(y_scale, dtype=F32)       # one fp32 product
        gz = torch.where(live, prod, torch.zeros_like(prod)).to(dt)
    gz_w, gz_x = gz.clone(), gz.clone()                              # what the weight / input gradient reads
    if variant == "drop_last_k":
        gz_w[-1, :] = 0
        gz_x[:, -1] = 0
    elif variant == "tail_from_8":
        gz_w[(B // 8) * 8:, :] = 0
        gz_x[:, (N // 8) * 8:] = 0
    elif variant == "row64_from_63":
        if N > 64:
            gz_w[:, 64] = gz_w[:, 63]
        if B > 64:
            gz_x[64] = gz_x[63]
    g_w = mm(gz_w.t().contiguous(), xs.t().contiguous())
    g_b = None
    if want_gb:
        g_b = mm(gz_w.t().contiguous(), torch.ones(1, B, dtype=dt))[:, 0]
        if variant == "bias_last_group":
            g_b[(N // 4) * 4:] = 0
    g_x = fac = gzr = wr = None
    if want_gx:
        gzr, wr = gz_x, ws
        if bf16:
            gzr, wr = (gz_x if variant == "gz_unrounded" else rnd(gz_x)), rnd(ws)
        g_x = mm(gzr, wr.t().contiguous())
        if gx_mask:
            scale = 1.0 if variant == "no_gx_scale" else gx_scale
            fac = torch.where(xs > 0, torch.full_like(xs, scale), torch.zeros_like(xs))
            g_x = g_x * fac
    if not want_bound:
        return Bwd((g_w, g_b, g_x), None)
    agz = gz.abs()
    b_w = (B + C_TAIL) * U * mm_exact(agz.t(), xs.abs().t())
    b_b = (B + C_TAIL) * U * agz.sum(0) if want_gb else None
    b_x = None
    if want_gx:
        b_x = (N + C_TAIL) * U * mm_exact(gzr.abs(), wr.abs().t())
        if gx_mask:
            b_x = b_x * fac
    return Bwd((g_w, g_b, g_x), (b_w, b_b, b_x))


# ------------------------------------------------------------------------------------------------------------ cases
def _f(S, B, K, N, **kw):
    d = dict(S=S, B=B, K=K, N=N, shared=True, relu=True, bias=True, p=0.0, off=0, counter=None, inc=0, math="f32",
             x16=False, y16=False)
    d.update(kw)
    return d


# (S, B, in = K, out = N).  GEMM rows: B when x is shared, S * B otherwise.  Rows 1 / 63 / 64 / 65 / 130 (129: a sample
# boundary inside a tile), out 1 / 3 / 4 / 63 / 64 / 65 / 130, in 1 / 7 / 8 / 12 / 31 / 32 / 33 / 40 / 64 / 65 / 100
# (one stage exactly, odd and even stage counts, valid < 8 in the last segment, a scalar-only row length).
FWD_CASES = {
    "m1-n1-k1":            _f(1, 1, 1, 1, relu=False),
    "m63-n3-k7":           _f(5, 63, 7, 3, p=0.5, off=17),                                     # runs of 3 and 2
    "m64-n4-k8":           _f(10, 64, 8, 4, bias=False, p=0.9, off=WRAP),                      # runs of 4, 4 and 2; the index wraps
    "m65-n63-k12":         _f(1, 65, 12, 63, shared=False, p=0.5, off=17, counter=5),
    "m130-n64-k31":        _f(1, 130, 31, 64, relu=False, bias=False),
    "m63-n65-k32":         _f(3, 21, 32, 65, shared=False, p=0.5, off=WRAP, counter=5),        # wraps through the counter
    "m64-n130-k33":        _f(5, 64, 33, 130, p=0.9),
    "m130-n4-k40-inc":     _f(2, 65, 40, 4, shared=False, counter=5, inc=3),                   # moves the counter, nothing else
    "m65-n64-k65":         _f(10, 65, 65, 64, p=0.5),
    "m1-n130-k100":        _f(5, 1, 100, 130, relu=False, p=0.5, off=17),
    "m129-n3-k64":         _f(3, 43, 64, 3, shared=False, p=0.5),
    "b-m63-n4-k12-x16":    _f(5, 63, 12, 4, math="bf16", x16=True, p=0.5),                     # W vector loads, x scalar loads
    "b-m64-n63-k8-x16-y16": _f(1, 64, 8, 63, math="bf16", shared=False, x16=True, y16=True),
    "b-m65-n64-k32-y16":   _f(10, 65, 32, 64, math="bf16", y16=True, bias=False, p=0.5, off=WRAP),
    "b-m130-n65-k33":      _f(2, 65, 33, 65, math="bf16", shared=False, relu=False, p=0.9),
    "b-m1-n1-k7-y16":      _f(1, 1, 7, 1, math="bf16", y16=True, relu=False),
    "b-m63-n130-k40-x16":  _f(3, 21, 40, 130, math="bf16", shared=False, x16=True, p=0.5, counter=5),
    "b-m130-n3-k100":      _f(5, 130, 100, 3, math="bf16"),
    "b-m65-n8-k64-x16":    _f(1, 65, 64, 8, math="bf16", shared=False, x16=True, p=0.5),
    "b-m64-n64-k31-y16":   _f(5, 64, 31, 64, math="bf16", y16=True, p=0.5, off=17),
    "b-m65-n12-k1-x16-y16": _f(1, 65, 1, 12, math="bf16", x16=True, y16=True, p=0.5),
    "b-m130-n4-k8-y16-inc": _f(2, 130, 8, 4, math="bf16", y16=True, counter=5, inc=3),
    # 32 x 18 = 576 tiles of 128 x 128: the one case on the big tile (every other plan says 64)
    "b-big-m3973-n2179-k40": _f(1, 3973, 40, 2179, math="bf16", shared=False),
}
BIG = "b-big-m3973-n2179-k40"


def _b(B, K, N, **kw):
    d = dict(B=B, K=K, N=N, y=True, y_scale=2.0, mask=True, gx_scale=2.0, gb=True, gx=True, math="f32")
    d.update(kw)
    return d


# (batch, in = K, out = N).  g_x reduces over out, g_w and g_b over batch: both walk 1 / 5 or 7 / 8 / 12 / 31 / 32 / 33 / 40 /
# 65 / 100; the batches include 1, 5, 33, 65, 77 and 130 (ragged above 64); every dimension sees 1, 3 or 5, 4, 63, 64, 65, 130.
BWD_CASES = {
    "b1-i1-o1":            _b(1, 1, 1, y=False, mask=False),
    "b5-i3-o7":            _b(5, 3, 7),
    "b33-i4-o8":           _b(33, 4, 8, mask=False),
    "b65-i63-o12":         _b(65, 63, 12, math="bf16"),
    "b77-i64-o31":         _b(77, 64, 31, y=False),
    "b130-i65-o32":        _b(130, 65, 32, gb=False),
    "b7-i130-o33":         _b(7, 130, 33, math="bf16", mask=False),
    "b8-i4-o40":           _b(8, 4, 40, gx=False),
    "b12-i64-o65":         _b(12, 64, 65, math="bf16", y=False),
    "b31-i8-o100":         _b(31, 8, 100),
    "b32-i12-o130":        _b(32, 12, 130, math="bf16"),
    "b40-i1-o64":          _b(40, 1, 64, mask=False),
    "b64-i3-o63":          _b(64, 3, 63, math="bf16", y=False, mask=False),
    "b100-i65-o4":         _b(100, 65, 4, gb=False, gx=False),
    "b63-i130-o3":         _b(63, 130, 3, math="bf16"),
    "b130-i40-o1":         _b(130, 40, 1, math="bf16"),
    "b1-i64-o64":          _b(1, 64, 64),
    "b65-i4-o65":          _b(65, 4, 65, y=False, mask=False, gb=False),
    "b33-i32-o33":         _b(33, 32, 33, math="bf16", gb=False),
    "b5-i63-o130":         _b(5, 63, 130, gx=False),
    "b77-i12-o12":         _b(77, 12, 12, math="bf16"),
    "b130-i130-o130":      _b(130, 130, 130),
    "b65-i8-o40":          _b(65, 8, 40, math="bf16", y=False, gb=False),
}


def _rs(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)


def _t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def fwd_rows(c):
    return c["B"] if c["shared"] else c["S"] * c["B"]


def fwd_sample0(c):
    """The global index of the launch's first sample, before the wrap."""
    return c["off"] + (c["counter"] or 0)


@functools.lru_cache(maxsize=None)
def fwd_inputs(name):
    """x (fp32, or bf16 when the case says so), w, b: x uniform in [-1, 1], W and b in [-0.5, 0.5]."""
    c, rs = FWD_CASES[name], _rs(name)
    S, B, K, N = c["S"], c["B"], c["K"], c["N"]
    x = _t32(rs.uniform(-1, 1, (B, K) if c["shared"] else (S, B, K)))
    if c["x16"]:
        x = x.to(torch.bfloat16)
    w = _t32(rs.uniform(-0.5, 0.5, (N, K)))
    b = _t32(rs.uniform(-0.5, 0.5, N)) if c["bias"] else None
    return dict(x=x, w=w, b=b)


@functools.lru_cache(maxsize=None)
def bwd_inputs(name):
    """x, gy uniform in [-1, 1], W in [-0.5, 0.5]; y uniform in [-1, 1] (half of it non-positive) with a twentieth exact zeros
    of either sign -- the first element among them -- and a positive last element."""
    c, rs = BWD_CASES[name], _rs(name)
    B, K, N = c["B"], c["K"], c["N"]
    x, gy, w = rs.uniform(-1, 1, (B, K)), rs.uniform(-1, 1, (B, N)), rs.uniform(-0.5, 0.5, (N, K))
    y = None
    if c["y"]:
        y = rs.uniform(-1, 1, (B, N))
        z = rs.uniform(size=y.shape)
        y[z < 0.025] = 0.0
        y[(z >= 0.025) & (z < 0.05)] = -0.0
        y[-1, -1] = abs(y[-1, -1]) + 0.25
        if y.size > 1:
            y.flat[0] = 0.0
        if y.size > 2:
            y.flat[1] = -0.0
        y = _t32(y)
    return dict(x=_t32(x), gy=_t32(gy), w=_t32(w), y=y)


def fwd_run(name, **kw):
    c, d = FWD_CASES[name], fwd_inputs(name)
    return fwd_ref(d["x"], d["w"], d["b"], S=c["S"], relu=c["relu"], drop_p=c["p"], sample0=fwd_sample0(c),
                   bf16=c["math"] == "bf16", y_bf16=c["y16"], **kw)


def bwd_run(name, **kw):
    c, d = BWD_CASES[name], bwd_inputs(name)
    return bwd_ref(d["x"], d["gy"], d["w"], d["y"], y_scale=c["y_scale"], gx_mask=c["mask"], gx_scale=c["gx_scale"],
                   bf16=c["math"] == "bf16", want_gb=c["gb"], want_gx=c["gx"], **kw)


@functools.lru_cache(maxsize=None)
def fwd_reference(name):
    """The fp64 reference of a case, computed once and shared; callers leave it unchanged."""
    return fwd_run(name)


@functools.lru_cache(maxsize=None)
def bwd_reference(name):
    return bwd_run(name)


# ------------------------------------------------------------------------------------------------------------ variants
FWD_VARIANTS = ("drop_last_k", "tail_from_8", "row64_from_63", "bias_last_group", "mask_shift_col", "mask_shift_sample",
                "bf16_trunc", "skip_last_run")
BWD_VARIANTS = ("drop_last_k", "tail_from_8", "row64_from_63", "bias_last_group", "y_ge", "no_y_scale", "no_gx_scale",
                "bf16_trunc", "gz_unrounded")


def fwd_applies(c, variant):
    return {
        "drop_last_k": True,
        "tail_from_8": c["K"] % 8 != 0,
        "row64_from_63": fwd_rows(c) > 64,
        "bias_last_group": c["bias"] and c["N"] % 4 != 0,
        "mask_shift_col": c["p"] > 0,
        "mask_shift_sample": c["p"] > 0,
        "bf16_trunc": c["math"] == "bf16",
        "skip_last_run": plan_runs(fwd_rows(c), c["N"], c["S"], c["shared"])[0] > 1,
    }[variant]


def bwd_applies(c, variant):
    B, N = c["B"], c["N"]
    return {
        "drop_last_k": True,
        "tail_from_8": B % 8 != 0 or (c["gx"] and N % 8 != 0),
        "row64_from_63": N > 64 or (c["gx"] and B > 64),
        "bias_last_group": c["gb"] and N % 4 != 0,
        "y_ge": c["y"] and B * N > 1,
        "no_y_scale": c["y"],
        "no_gx_scale": c["mask"] and c["gx"],
        "bf16_trunc": c["math"] == "bf16" and c["gx"],
        "gz_unrounded": c["math"] == "bf16" and c["gx"],
    }[variant]


# ------------------------------------------------------------------------------------------------------------ shares
def _share(err, bound):
    sh = torch.where(err == 0, torch.zeros_like(err), err / bound)          # (x / 0 = inf; NaN stays NaN)
    sh = torch.where(torch.isnan(sh), torch.full_like(sh, float("inf")), sh)
    return float(sh.max()) if sh.numel() else 0.0


def fwd_share(got, ref):
    """Largest |got - ref| / bound over the elements (0 / 0 counts as 0; a NaN, or an error over a zero bound, as inf).  A
    bf16 y: the distance from the middle of [bf16(lo), bf16(hi)] over its half width -- at most 1 exactly when inside."""
    got = got.detach().cpu().to(F64)
    if ref.lo is None:
        return _share((got - ref.y).abs(), ref.bound)
    return _share((got - (ref.lo + ref.hi) / 2).abs(), (ref.hi - ref.lo) / 2)


def bwd_shares(got, ref):
    """Per tensor of (g_w, g_b, g_x): as fwd_share; None where the case has no such output."""
    return [None if r is None else _share((g.detach().cpu().to(F64) - r).abs(), b)
            for g, r, b in zip(got, ref.grads, ref.bounds)]
