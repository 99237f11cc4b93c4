"""TEST INFRASTRUCTURE: fp64 restatement of ONE launch of the fused optimiser steps (bnn_adam_step: csrc/optim.hip;
bnn_sgd_step: csrc/dense_train.hip; the chunk walk ChunkList of csrc/bnn_device.h) with a derived error bound for EVERY
output element, an fp32 emulation of the kernels' arithmetic, the seeded wrong variants the bound has to reject, and the
table of cases shared by tests/test_optim_cpu.py and tests/test_gpu_optim.py.  numpy / torch-CPU only: imports without a
GPU.

What is restated
----------------
From the launch's actual fp32 inputs (p, g, m, v) -- g possibly bf16 values, widened -- and the scalars as the caller
gave them (doubles; a learning rate read from a device word is the fp32 number in that word), torch's
_single_tensor_adam in fp64:
    gg = g + wd p        m' = m + (gg - m)(1 - b1)        v' = b2 v + (1 - b2) gg^2
    bc1 = 1 - b1^step    bc2 = 1 - b2^step                denom = sqrt(v') / sqrt(bc2) + eps
    s = lr / bc1         D = s m' / denom                 p' = p - D
and for SGD  p' = p - lr (g + wd p).  v' = 0 with eps = 0 is 0 / 0 in the rule itself: the cases hold no such element.

The bound
---------
u = 2^-24 is the unit roundoff of fp32 round-to-nearest: fl(x) = x (1 + d), |d| <= u, for +, -, *, /, sqrt, fma and the
double -> float casts (division and square root are correctly rounded in this build).  The kernel's roundings, in the
order of optim.hip, each charged against the absolute value of what it rounds, errors of earlier results carried forward
by first-order propagation (so a cancelling gg - m, m' or g + wd p is covered by the propagated absolute terms, never by
a relative figure on the small result):

  gg   (wd != 0 only) cast of wd, the fma:                       d_gg = u (|wd p| + |gg|)                       [2]
  m'   the subtract gg - m, the cast of 1 - b1, the fma:         d_m  = u |m'| + (1 - b1) (2 u |gg - m| + d_gg)  [3]
  v'   casts of 1 - b2 and b2, the products (1 - b2) gg and (.) gg, the fma:
                                                                 d_v  = u v' + u b2 v + 3 u (1 - b2) gg^2
                                                                        + (1 - b2) (2 |gg| d_gg + d_gg^2)         [5]
  denom  R = sqrt(v') / sqrt(bc2): the sqrt, the cast of sqrt(bc2), the quotient; the cast of eps; the add:
                                                                 d_den = u denom + u eps + (3 u + e2) R
                                                                         + d_v / (2 sqrt(v') sqrt(bc2))          [5]
  p'   the cast of s, the quotient m' / denom, the product, the subtract:
                                                                 d_p  = u |p'| + (1 + u) ((3 u + e1) |D|
                                                                        + s d_m / denom + |D| d_den / denom)      [4]
       (-ffp-contract=fast fuses the product and the subtract into one fma in the compiled kernel, and the emulation
       below follows it: one rounding fewer.  The bound keeps the count of the source as written.)

e1, e2 are the double-precision bias corrections: pow within 16 ulp (the OpenCL bound of the device library; the host's
is below 1), the subtract, the quotient / square root, on both sides of the comparison:
e = (2^-48 b^step + 2^-50) / bc -- at most 1e-11, it never decides anything.  Each bound also carries k * 2^-150 for its
k roundings (half the spacing of the fp32 subnormals: what a rounding that underflows costs); no case underflows.

SGD (two fmas; the cast of lr -- a device word needs none, it is counted all the same --, and with wd != 0 the cast of
wd and the inner fma):   d_p = u |p'| + lr (u |gg| + d_gg).

Every constant above is the count of roundings, not the count times a safety factor, and none is measured.
tests/test_optim_cpu.py shows the fp32 emulation below inside the bound at every case (p': up to 0.997 of it, the final
half-ulp rounding of p' alone; m': up to 0.99985, the final rounding of an m' just above a power of two with a small
gg - m; v': up to 0.76) and every seeded wrong variant far outside it.

The emulation
-------------
adam_emul / sgd_emul: the kernels' fp32 arithmetic in numpy float32, same operation order, an fma as the exact fp64
product plus the addend rounded once to fp64 and then to fp32 (the double rounding differs from a true fma in about one
result in 2^29).  Used by the CPU tests only; `variant` selects a seeded wrong kernel (ADAM_VARIANTS, SGD_VARIANTS).
"""
import functools
import itertools
import math
import zlib

import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -150
F32, F64 = np.float32, np.float64
CHUNK = 4096              # kStreamChunk (csrc/bnn_stream.h)
MAX_TENSORS = 16          # BNN_ADAM_MAX_TENSORS, BNN_SGD_MAX_TENSORS
GUARD = 64                # floats of sentinel before and after every tensor
SENTINEL = 0xFFC5A5A5     # a NaN with a payload: an out-of-range READ shows as well (0xFFC5 is a bf16 NaN too)
NAMES = ("p", "m", "v")

ADAM_VARIANTS = ("no_eps", "eps_in_sqrt", "no_bc2", "no_bc1", "step_plus_1", "powf", "step_size_1.001", "adamw", "wd_ignored",
                 "last_unwritten", "group_from_chunk0")
SGD_VARIANTS = ("wd_ignored", "plus_lr", "lr_bf16")


def bf16r(a):
    """fp32 -> bf16 round-to-nearest-even, widened again (numpy float32)."""
    return torch.from_numpy(np.array(a, dtype=F32)).to(torch.bfloat16).to(torch.float32).numpy()


# ------------------------------------------------------------------------------------------------------------ fp64
def _e64(b, step, bc):
    return (2.0 ** -48 * b ** step + 2.0 ** -50) / bc


def adam_ref(p, g, m, v, *, lr, b1, b2, eps, wd, step, want_bound=True):
    """((p', m', v'), (bound_p, bound_m, bound_v)) of one launch, fp64."""
    p, g, m, v = (np.asarray(a, dtype=F64) for a in (p, g, m, v))
    lr, b1, b2, eps, wd, step = float(lr), float(b1), float(b2), float(eps), float(wd), int(step)
    gg = g + wd * p
    m1 = m + (gg - m) * (1.0 - b1)
    v1 = b2 * v + (1.0 - b2) * gg * gg
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    sq = np.sqrt(v1)
    R = sq / math.sqrt(bc2)
    denom = R + eps
    s = lr / bc1
    with np.errstate(divide="ignore", invalid="ignore"):
        D = s * m1 / denom
        p1 = p - D
        if not want_bound:
            return (p1, m1, v1), None
        d_gg = U * (np.abs(wd * p) + np.abs(gg)) if wd != 0.0 else np.zeros_like(gg)
        d_m = U * np.abs(m1) + (1.0 - b1) * (2 * U * np.abs(gg - m) + d_gg)
        d_v = U * v1 + U * b2 * v + 3 * U * (1.0 - b2) * gg * gg + (1.0 - b2) * (2 * np.abs(gg) * d_gg + d_gg * d_gg)
        prop = np.where(v1 > 0, d_v / (2 * sq * math.sqrt(bc2)), 0.0)
        d_den = U * denom + U * eps + (3 * U + _e64(b2, step, bc2)) * R + prop
        rest = (3 * U + _e64(b1, step, bc1)) * np.abs(D) + s * d_m / denom + np.abs(D) * d_den / denom
        d_p = U * np.abs(p1) + (1 + U) * rest
    return (p1, m1, v1), (d_p + 4 * TINY, d_m + 3 * TINY, d_v + 5 * TINY)


def sgd_ref(p, g, *, lr, wd, want_bound=True):
    """(p', bound_p) of one launch, fp64."""
    p, g = np.asarray(p, dtype=F64), np.asarray(g, dtype=F64)
    lr, wd = float(lr), float(wd)
    gg = g + wd * p
    p1 = p - lr * gg
    if not want_bound:
        return p1, None
    d_gg = U * (np.abs(wd * p) + np.abs(gg)) if wd != 0.0 else 0.0
    return p1, U * np.abs(p1) + lr * (U * np.abs(gg) + d_gg) + 2 * TINY


# ------------------------------------------------------------------------------------------------------------ fp32
def _fma(a, b, c):
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def adam_emul(p, g, m, v, *, lr, b1, b2, eps, wd, step, variant=None):
    """(p', m', v') float32: the arithmetic of adam_kernel's element body, or a seeded wrong one."""
    p, g, m, v = (np.asarray(a, dtype=F32) for a in (p, g, m, v))
    wdf, epsf, b2f = F32(wd), F32(eps), F32(b2)
    omb1, omb2 = F32(1.0 - b1), F32(1.0 - b2)
    st = step + 1 if variant == "step_plus_1" else step
    if variant == "powf":
        bc1 = float(F32(1) - np.power(F32(b1), F32(st)))
        bc2 = float(F32(1) - np.power(F32(b2), F32(st)))
    else:
        bc1, bc2 = 1.0 - float(b1) ** st, 1.0 - float(b2) ** st
    if variant == "no_bc1":
        bc1 = 1.0
    if variant == "no_bc2":
        bc2 = 1.0
    step_size = F32(float(lr) / bc1 * (1.001 if variant == "step_size_1.001" else 1.0))
    sqrt_bc2 = F32(math.sqrt(bc2))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        if variant == "adamw":
            p = (p * F32(1.0 - float(lr) * float(wd))).astype(F32)
        gg = _fma(wdf, p, g) if wdf != 0 and variant not in ("adamw", "wd_ignored") else g
        m1 = _fma(gg - m, omb1, m)
        v1 = _fma(v, b2f, omb2 * gg * gg)
        if variant == "eps_in_sqrt":
            denom = np.sqrt(v1 + epsf) / sqrt_bc2
        elif variant == "no_eps":
            denom = np.sqrt(v1) / sqrt_bc2
        else:
            denom = np.sqrt(v1) / sqrt_bc2 + epsf
        p1 = _fma(-step_size, m1 / denom, p)              # the compiled kernel: product and subtract contracted
    assert p1.dtype == F32 and m1.dtype == F32 and v1.dtype == F32 and denom.dtype == F32
    return p1, m1, v1


def sgd_emul(p, g, *, lr, wd, variant=None):
    p, g = np.asarray(p, dtype=F32), np.asarray(g, dtype=F32)
    lrf = F32(lr)
    if variant == "lr_bf16":
        lrf = bf16r(np.array([lrf]))[0]
    nlr = lrf if variant == "plus_lr" else -lrf
    wdf = F32(0.0 if variant == "wd_ignored" else wd)
    return _fma(nlr, _fma(wdf, p, g) if wdf != 0 else g, p)


def adam_emul_list(tensors, scal, variant=None):
    """adam_emul over a call's tensors; the two geometry variants act here."""
    out = []
    for t in tensors:
        o = [a.copy() for a in adam_emul(t["p"], t["g"], t["m"], t["v"], variant=variant, **scal)]
        n = o[0].size
        if variant == "last_unwritten":
            for a, src in zip(o, (t["p"], t["m"], t["v"])):
                a[-1] = src[-1]
        elif variant == "group_from_chunk0" and n >= CHUNK + 4:
            for a, b in zip(o, adam_emul(t["p"][:4], t["g"][:4], t["m"][:4], t["v"][:4], **scal)):
                a[CHUNK:CHUNK + 4] = b
        out.append(tuple(o))
    return out


# ------------------------------------------------------------------------------------------------------------ chunks
def chunk_table(sizes, chunk=CHUNK):
    """ChunkList restated: per block of ONE launch (tensor, first element, elements) -- add() / finish() / find()."""
    assert 0 < len(sizes) <= MAX_TENSORS and all(n > 0 for n in sizes)
    first = [0]
    for n in sizes:
        first.append(first[-1] + (n + chunk - 1) // chunk)
    blocks = []
    for b in range(first[-1]):
        t = 0
        while t + 1 < len(sizes) and b >= first[t + 1]:
            t += 1
        base = (b - first[t]) * chunk
        blocks.append((t, base, min(chunk, sizes[t] - base)))
    return blocks


def launches(sizes):
    """The tensor counts of a call's launches (16 tensors per launch)."""
    return [sizes[lo:lo + MAX_TENSORS] for lo in range(0, len(sizes), MAX_TENSORS)]


def block_kind(sizes, block):
    """'whole' (the fast body), 'full4' (general loop ending on a full group of four), 'ragged' (scalar tail)."""
    t, base, cnt = block
    if base + CHUNK <= sizes[t]:
        return "whole"
    return "full4" if cnt % 4 == 0 else "ragged"


# ------------------------------------------------------------------------------------------------------------ cases
GEO16 = (1, 4097, 3, 4096, 5, 4095, 8193, 7, 8192, 4, 8191, 12289, 2, 1025, 33 * 5, 1)
GEO19 = GEO16 + (4100, 6, 37)       # 4100: a later chunk that ends on a full group of four
GEO17 = GEO16 + (4100,)
GRIDS = {1: (777,), 2: (4097,), 7: (4096, 8193, 3, 8191), 8: (4096, 8193, 3, 8191, 100), 9: (12289, 4097, 5, 8192),
         16: (12289, 4097, 5, 8192, 16385, 4095, 1), 17: (12289, 4097, 5, 8192, 16385, 4095, 1, 2)}
REGIME_N = 4099           # a whole chunk, then a tail chunk of 3: the scalar tail alone; 4-wide tails are in the geometry
STEPS = (1, 2, 7, 1000, 10 ** 6, 2 ** 32 - 1)
WDS = (0.0, 0.01)
EPSS = (1e-8, 0.0, 1e-3)
BETAS = ((0.9, 0.999), (0.0, 0.999), (0.9, 0.0))
LR = 1e-3                 # not an fp32 number: the host path keeps the double
LR32 = float(F32(1e-3))   # where launch forms are compared in bits, and what a device word holds


def _case(sizes, step, wd=0.0, eps=1e-8, betas=BETAS[0], lr=LR):
    return dict(sizes=tuple(sizes), step=step, wd=wd, eps=eps, b1=betas[0], b2=betas[1], lr=lr)


REGIMES = {f"s{st}-wd{wd:g}-eps{eps:g}-b{b[0]:g}_{b[1]:g}": _case((REGIME_N,), st, wd, eps, b)
           for st, wd, eps, b in itertools.product(STEPS, WDS, EPSS, BETAS)}
GEOMETRY = {"geo16": _case(GEO16, 7, 0.01), "geo19": _case(GEO19, 1000, 0.0), "geo16-step1": _case(GEO16, 1, 0.0),
            **{f"grid{n}": _case(s, 2, 0.01 if n % 2 else 0.0) for n, s in GRIDS.items()}}
ADAM_CASES = {**REGIMES, **GEOMETRY}
SGD_LR = 0.0371
SGD_CASES = {f"sgd-{nm}-wd{wd:g}": dict(sizes=tuple(s), lr=SGD_LR, wd=wd)
             for (nm, s), wd in itertools.product((("regime", (REGIME_N,)), ("geo16", GEO16), ("geo17", GEO17)), (0.0, 1e-3))}
assert all(sum(c["sizes"]) <= 60000 for c in list(ADAM_CASES.values()) + list(SGD_CASES.values()))

# element kinds of the inputs, by index % 32 (index 4096, 4097, 4098 of the regime tensor -- its scalar tail -- are 0, 1, 2)
K_ZERO, K_GZERO, K_CANCEL, K_PZERO, K_PSMALL = 0, 1, 2, 3, 4


def scalars(c):
    return {k: c[k] for k in ("lr", "b1", "b2", "eps", "wd", "step")}


def _rs(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)


def _tensor(rs, n, step, wd, eps, b1, b2):
    sign = lambda: rs.choice([-1.0, 1.0], n)
    g = sign() * 10.0 ** rs.uniform(-10.0, 2.0, n)
    # 25 % of p as a network's weights are, 75 % small: there the update is seen at its own precision, not at ulp(p)
    p = np.where(rs.uniform(size=n) < 0.25, rs.standard_normal(n) * rs.choice([0.1, 1.0, 5.0], n),
                 sign() * 10.0 ** rs.uniform(-10.0, 0.0, n))
    # the moments a run would hold after step - 1 steps of such gradients: the bias the corrections of this step undo
    m = g * rs.uniform(-1.0, 1.0, n) * (1.0 - b1 ** max(step - 1, 1))
    v = g * g * rs.uniform(0.25, 4.0, n) * (1.0 - b2 ** max(step - 1, 1))
    a = rs.randint(1, 16, n) * 2.0 ** rs.randint(-30, 0, n)          # <= 4 bits: 9 a is exact in fp32 and in bf16
    small = sign() * rs.uniform(0.0, 1e-6, n)
    kind = np.arange(n) % 32
    if step == 1:
        m[:], v[:] = 0.0, 0.0
    if eps > 0:                                                       # with eps = 0 the rule itself gives 0 / 0 here
        z = kind == K_ZERO
        g[z], m[z], v[z] = 0.0, 0.0, 0.0
        if wd != 0:
            p[z] = 0.0
    if step > 1 and (eps > 0 or b2 > 0):                              # (eps = 0 and b2 = 0: v' = gg^2 = 0, m' / 0)
        g[kind == K_GZERO] = 0.0
    if step > 1 and b1 == 0.9:                                        # m = -(1 - b1) gg / b1 = -gg / 9: m' cancels
        c = kind == K_CANCEL
        g[c], m[c], p[c] = 9.0 * a[c], -a[c], 0.0
    p[kind == K_PZERO] = 0.0
    ps = kind == K_PSMALL
    p[ps] = small[ps]
    return {k: np.ascontiguousarray(x, dtype=F32) for k, x in (("p", p), ("g", g), ("m", m), ("v", v))}


def _freeze(ts):
    for t in ts:
        for a in t.values():
            a.setflags(write=False)
    return ts


@functools.lru_cache(maxsize=None)
def adam_inputs(name, bf16=False):
    """The tensors of a case: a tuple of dicts of read-only fp32 arrays p, g, m, v.  bf16: g rounded to bf16 (widened)."""
    c = ADAM_CASES[name]
    rs = _rs(name)
    ts = [_tensor(rs, n, c["step"], c["wd"], c["eps"], c["b1"], c["b2"]) for n in c["sizes"]]
    if bf16:
        for t in ts:
            t["g"] = bf16r(t["g"])
    return tuple(_freeze(ts))


@functools.lru_cache(maxsize=None)
def sgd_inputs(name):
    c = SGD_CASES[name]
    rs = _rs(name)
    return tuple(_freeze([_tensor(rs, n, 2, c["wd"], 1.0, 0.9, 0.999) for n in c["sizes"]]))


@functools.lru_cache(maxsize=None)
def adam_expected(name, bf16=False):
    """Per tensor ((p', m', v'), bounds) of the case's one call, computed once."""
    c = ADAM_CASES[name]
    return tuple(adam_ref(t["p"], t["g"], t["m"], t["v"], **scalars(c)) for t in adam_inputs(name, bf16))


@functools.lru_cache(maxsize=None)
def sgd_expected(name, lr=None):
    c = SGD_CASES[name]
    return tuple(sgd_ref(t["p"], t["g"], lr=c["lr"] if lr is None else lr, wd=c["wd"]) for t in sgd_inputs(name))


def share(got, ref, bound):
    """Largest |got - ref| / bound over the elements (0 / 0 counts as 0; a NaN, or an error over a zero bound, as inf)."""
    got = np.asarray(got, dtype=F64)
    if got.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.abs(got - ref)
        sh = np.where(err == 0, 0.0, err / bound)
    sh = np.where(np.isnan(sh) | np.isnan(got), np.inf, sh)
    return float(sh.max())


def adam_shares(got, expected):
    """got: per tensor (p', m', v'); the worst share per output over the call's tensors, as a dict p / m / v."""
    worst = dict.fromkeys(NAMES, 0.0)
    assert len(got) == len(expected)
    for o, (ref, bound) in zip(got, expected):
        for k, a, r, b in zip(NAMES, o, ref, bound):
            assert np.asarray(a).shape == r.shape
            worst[k] = max(worst[k], share(a, r, b))
    return worst


def sgd_share(got, expected):
    assert len(got) == len(expected)
    return max(share(a, r, b) for a, (r, b) in zip(got, expected))


# ------------------------------------------------------------------------------------------------------------ guards
def arena(arrays, itemsize=4):
    """One buffer for a call's arrays of one kind: every array a 16-byte-aligned view, GUARD floats of SENTINEL before and
    after it.  arrays: numpy float32 (itemsize 4), or float32 holding bf16 values (itemsize 2: stored as their upper 16
    bits).  Returns (image, spans): image a numpy uint32 / uint16 array, spans the (offset, count) of every view."""
    per = 4 // itemsize
    guard, align = GUARD * per, 16 // itemsize
    dt, fill = (np.uint32, SENTINEL) if itemsize == 4 else (np.uint16, SENTINEL >> 16)
    spans, off = [], guard
    for a in arrays:
        spans.append((off, a.size))
        off += -(-a.size // align) * align + guard
    image = np.full(off, fill, dtype=dt)
    for (o, n), a in zip(spans, arrays):
        bits = np.ascontiguousarray(a, dtype=F32).view(np.uint32)
        if itemsize == 2:
            assert not (bits & 0xFFFF).any(), "not bf16 values"
            bits = (bits >> 16).astype(np.uint16)
        image[o:o + n] = bits
    return image, spans


def arena_guards_intact(image, spans):
    """True when every word of `image` outside the spans still holds the sentinel."""
    fill = SENTINEL if image.dtype == np.uint32 else SENTINEL >> 16
    outside = np.ones(image.size, dtype=bool)
    for o, n in spans:
        outside[o:o + n] = False
    return bool((image[outside] == fill).all())
