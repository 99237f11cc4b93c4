"""K5 bnn_dense_fwd (csrc/mlp_dropout.hip) and K6 bnn_dense_bwd (csrc/dense_train.hip, csrc/dense_tile.h) on an MI355X
against the fp64 restatement tests/dense_layer_ref.py: EVERY element of every output under its own bound (the derivation is
that module's docstring; tests/test_dense_layer_cpu.py proves the restatement against autograd, the bound wide enough for
fp32 in three orders and tight enough for the seeded wrong variants), over the table of that module.  Every output sits
NaN-filled between two sentinel blocks that have to come back bit-unchanged, and every case whose row lengths are
multiples of 4 runs again with each operand and each output in turn off its 16-byte (bf16: 16- and 8-byte) boundary -- the
scalar load / store paths torch's own allocations never reach -- and has to give the same bits.  Then the bit-equality
promises of the kernels' own comments: one launch against single-sample launches, shared x against repeated x, the
128 x 128 tile against the 64 x 64 tile, BF16X3 against F32, the device counter against the offset, and g_w / g_b / g_x
whatever other outputs are asked for.  Public ops entry points only.

Measured on an MI355X on 2026-10-21, after the bound and the table were fixed, and used as no threshold (largest
|got - ref| / bound over a tensor's elements, over the cases of a math mode):
                        y       g_w     g_b     g_x
  bnn_dense_fwd  f32    0.079                           (m130-n64-k31)
  bnn_dense_fwd  bf16   0.031                           (fp32 y; the 128 x 128-tile case)
  bnn_dense_bwd  f32            0.094   0.066   0.068
  bnn_dense_bwd  bf16           0.100   0.048   0.048   (g_w and g_b are fp32 GEMMs in every mode)
A bf16 y: all 67 933 elements of the six cases equal bf16(ref) itself, the ties (0.47 % .. 0.66 % of a case) included.
Every bit-equality below held at the first run; no kernel was changed.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import dense_layer_ref as R
from bnn_hip import _lib as L
from bnn_hip import ops

PAD = 64                       # sentinel elements on either side: 256 bytes of fp32, 128 of bf16, so offsets count from 16-byte boundaries
F64 = torch.float64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------------ placement
def _ints(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _pattern(n, like):
    """A sentinel pattern of n elements in `like`'s integer view (fp32: mostly NaNs and huge numbers, never a plausible value)."""
    i = torch.arange(n, dtype=torch.int64)
    if like.element_size() == 4:
        return (0x7FC00000 + (i * 7919) % 0x3FFFFF).to(torch.int32)
    return (0x7FC0 + (i * 13) % 0x3F).to(torch.int16)


class Slot:
    """A contiguous view of a tensor's shape `off` elements past a 16-byte boundary inside a larger buffer of sentinels.
    value None: the extent is filled with NaN (an output)."""

    def __init__(self, dev, shape, dtype, value=None, off=0):
        n = 1
        for s in shape:
            n *= s
        self.lo, self.n = PAD + off, n
        self.buf = torch.empty(self.lo + n + PAD, dtype=dtype, device=dev)
        self.want = _pattern(self.buf.numel(), self.buf).to(dev)
        _ints(self.buf).copy_(self.want)
        self.t = self.buf[self.lo:self.lo + n].view(shape)
        assert self.buf.data_ptr() % 256 == 0 and self.t.is_contiguous()
        assert self.t.data_ptr() % 16 == (off * self.buf.element_size()) % 16
        if value is None:
            self.t.fill_(float("nan"))
        else:
            self.t.copy_(value)

    def intact(self):
        got = _ints(self.buf)
        return torch.equal(got[:self.lo], self.want[:self.lo]) and torch.equal(got[self.lo + self.n:], self.want[self.lo + self.n:])


def _slot(dev, value, off=0):
    return None if value is None else Slot(dev, tuple(value.shape), value.dtype, value, off)


def _t(slot):
    return None if slot is None else slot.t


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_ints(a.contiguous()), _ints(b.contiguous()))


def _math(c, x3=False):
    if c["math"] == "bf16":
        return L.MATH_BF16
    return L.MATH_BF16X3 if x3 else L.MATH_F32


# ------------------------------------------------------------------------------------------------------------ forward
def _fwd(dev, name, place=None, x_value=None, x3=False, plan=False, **over):
    """One bnn_dense_fwd launch of case `name`, its fields overridden by `over`.  place: element offsets of x / w / b / y off
    their 16-byte boundaries; x_value: another x.  Returns (y, the counter's value after the launch), or the launch's plan."""
    c = dict(R.FWD_CASES[name], **over)
    d = R.fwd_inputs(name)
    place = place or {}
    x = d["x"] if x_value is None else x_value
    S = c["S"]
    B, N = x.shape[-2], c["N"]
    values = (x, d["w"], d["b"])
    ins = [_slot(dev, v, place.get(k, 0)) for k, v in zip("xwb", values)]
    y = Slot(dev, (S, B, N), torch.bfloat16 if c["y16"] else torch.float32, None, place.get("y", 0))
    counter = None if c["counter"] is None else torch.tensor([c["counter"]], dtype=torch.int32, device=dev)
    kw = dict(n_samples=S, math_mode=_math(c, x3), relu=c["relu"], drop_p=c["p"], layer_id=R.LAYER_ID, seed=R.SEED,
              sample_offset=c["off"], sample_counter=counter, sample_counter_inc=c["inc"], out=y.t)
    if plan:
        return ops.dense_plan(_t(ins[0]), _t(ins[1]), _t(ins[2]), **kw)
    ops.dense_fwd(_t(ins[0]), _t(ins[1]), _t(ins[2]), **kw)
    torch.cuda.synchronize()
    assert y.intact(), (name, place, "a store outside y")
    for s, v in zip(ins, values):
        assert s is None or (s.intact() and _same_bits(s.t.cpu(), v)), (name, place, "an input changed")
    return y.t, None if counter is None else int(counter.item())


@functools.lru_cache(maxsize=None)
def _fwd_aligned(dev, name):
    return _fwd(dev, name)


def _fwd_offsets(c):
    """The misaligned placements of a case: each operand / output whose row length is a multiple of 4, in turn.  fp32: one
    float past a 16-byte boundary.  bf16: one element past a 16-byte boundary, on an 8-byte boundary that is no 16-byte one,
    and one element past that."""
    out = []
    if c["K"] % 4 == 0:
        out += [{"x": o} for o in ((1, 4, 5) if c["x16"] else (1,))] + [{"w": 1}]
    if c["N"] % 4 == 0:
        out += [{"y": o} for o in ((1, 4, 5) if c["y16"] else (1,))]
        if c["bias"]:
            out += [{"b": 1}]
    return out


@pytest.mark.parametrize("name", list(R.FWD_CASES))
def test_forward_within_the_fp64_bound(dev, name):
    c, ref = R.FWD_CASES[name], R.fwd_reference(name)
    plan = _fwd(dev, name, plan=True)
    assert plan["batch_rows"] == plan["features_per_block"] == (128 if name == R.BIG else 64)
    if name != R.BIG:
        assert plan["k_slices"] == R.plan_runs(R.fwd_rows(c), c["N"], c["S"], c["shared"])[0]
    y, counter = _fwd_aligned(dev, name)
    assert not bool(torch.isnan(y).any()), "an element of y was not written"
    share = R.fwd_share(y, ref)
    if c["y16"]:         # (the share of a bf16 y is its place between the two admissible ends: 1 on an end, and says little)
        off = int((y.cpu().to(F64) != R.bf16r(ref.y)).sum())
        print(f"dense_fwd {c['math']:4s} y16 {name:24s} inside [bf16(lo), bf16(hi)]: {share <= 1.0}; {off} of {y.numel()} elements "
              f"are not bf16(ref); ties {ref.info['tie_share']:.4f}")
    else:
        print(f"dense_fwd {c['math']:4s} y32 {name:24s} share of the bound {share:.3f}")
    assert share <= 1.0, (name, share)
    if c["counter"] is not None:
        assert counter == c["counter"] + c["inc"]
    for off in _fwd_offsets(c):
        y1, counter1 = _fwd(dev, name, place=off)
        assert _same_bits(y1, y), (name, off, "misaligned run differs from the aligned run")
        assert counter1 == counter


ONE_BY_ONE = ["m64-n4-k8", "m63-n65-k32", "m65-n64-k65", "b-m65-n64-k32-y16", "b-m63-n130-k40-x16", "m63-n3-k7"]


@pytest.mark.parametrize("name", ONE_BY_ONE)
def test_one_launch_equals_single_sample_launches(dev, name):
    """S samples in one launch against the same samples in S launches of one sample at sample_offset + counter + s (mod
    2^32), with no counter: the split of the samples over calls and over a shared-x launch's runs changes no bit."""
    c, d = R.FWD_CASES[name], R.fwd_inputs(name)
    y, _ = _fwd_aligned(dev, name)
    for s in range(c["S"]):
        xs = d["x"] if c["shared"] else d["x"][s:s + 1].contiguous()
        ys, _ = _fwd(dev, name, x_value=xs, S=1, off=(R.fwd_sample0(c) + s) & 0xFFFFFFFF, counter=None)
        assert _same_bits(ys[0], y[s]), (name, s)


@pytest.mark.parametrize("name", ["m63-n3-k7", "m64-n4-k8", "m65-n64-k65", "b-m63-n4-k12-x16", "b-m65-n64-k32-y16"])
def test_shared_x_equals_repeated_x(dev, name):
    c, d = R.FWD_CASES[name], R.fwd_inputs(name)
    assert c["shared"]
    y, _ = _fwd_aligned(dev, name)
    y1, _ = _fwd(dev, name, x_value=d["x"].unsqueeze(0).repeat(c["S"], 1, 1).contiguous())
    assert _same_bits(y1, y)


@pytest.mark.parametrize("name", [n for n, c in R.FWD_CASES.items() if c["counter"] is not None and not c["inc"]])
def test_device_counter_equals_the_offset(dev, name):
    c = R.FWD_CASES[name]
    y, counter = _fwd_aligned(dev, name)
    assert counter == c["counter"]                      # a drawing launch leaves the counter alone
    y1, _ = _fwd(dev, name, off=(c["off"] + c["counter"]) & 0xFFFFFFFF, counter=None)
    assert _same_bits(y1, y)


@pytest.mark.parametrize("name", [n for n, c in R.FWD_CASES.items() if c["inc"]])
def test_counter_increment_changes_nothing_else(dev, name):
    y, counter = _fwd_aligned(dev, name)
    y1, _ = _fwd(dev, name, inc=0, counter=None)
    assert _same_bits(y1, y) and counter == R.FWD_CASES[name]["counter"] + R.FWD_CASES[name]["inc"]


@pytest.mark.parametrize("name", [n for n, c in R.FWD_CASES.items() if c["math"] == "f32"])
def test_forward_bf16x3_equals_f32(dev, name):
    y, _ = _fwd_aligned(dev, name)
    y1, _ = _fwd(dev, name, x3=True)
    assert _same_bits(y1, y)


def test_big_tile_rows_equal_small_tile_launches(dev):
    """Rows [0, 64) and [3968, 3973) of the 128 x 128-tile launch against the same rows computed by launches of their own,
    which take the 64 x 64 tile: an element is the same chain of MFMAs whatever the plan's tile."""
    c, d = R.FWD_CASES[R.BIG], R.fwd_inputs(R.BIG)
    y, _ = _fwd_aligned(dev, R.BIG)
    for lo, hi in ((0, 64), (3968, 3973)):
        xs = d["x"][:, lo:hi].contiguous()
        assert _fwd(dev, R.BIG, x_value=xs, plan=True)["batch_rows"] == 64
        ys, _ = _fwd(dev, R.BIG, x_value=xs)
        assert _same_bits(ys[0], y[0, lo:hi]), (lo, hi)


@pytest.mark.parametrize("x16,y16", [(False, False), (True, False), (False, True), (True, True)])
def test_big_tile_equals_small_tile_in_every_dtype(dev, x16, y16):
    """Every row of the 128 x 128-tile launch, in each of its four instantiations (x and y in fp32 or bf16), against 1024-row
    launches of the same rows (8 x 18 = 144 big tiles: below the threshold, so they take the 64 x 64 tile)."""
    d = R.fwd_inputs(R.BIG)
    x = d["x"].to(torch.bfloat16) if x16 else d["x"]
    assert _fwd(dev, R.BIG, x_value=x, y16=y16, plan=True)["batch_rows"] == 128
    y = _fwd_aligned(dev, R.BIG)[0] if not (x16 or y16) else _fwd(dev, R.BIG, x_value=x, y16=y16)[0]
    assert not bool(torch.isnan(y).any())
    for lo in range(0, x.shape[1], 1024):
        xs = x[:, lo:lo + 1024].contiguous()
        assert _fwd(dev, R.BIG, x_value=xs, y16=y16, plan=True)["batch_rows"] == 64
        ys, _ = _fwd(dev, R.BIG, x_value=xs, y16=y16)
        assert _same_bits(ys[0], y[0, lo:lo + 1024]), lo


# ------------------------------------------------------------------------------------------------------------ backward
def _bwd(dev, name, off=None, x3=False, **over):
    """One bnn_dense_bwd launch of case `name`: (g_w, g_b, g_x), None where the case (or `over`) asks for none."""
    c = dict(R.BWD_CASES[name], **over)
    d = R.bwd_inputs(name)
    off = off or {}
    B, K, N = c["B"], c["K"], c["N"]
    names = ("x", "gy", "w", "y")
    ins = {k: _slot(dev, d[k], off.get(k, 0)) for k in names}
    f32 = torch.float32
    outs = {"g_w": Slot(dev, (N, K), f32, None, off.get("g_w", 0)),
            "g_b": Slot(dev, (N,), f32, None, off.get("g_b", 0)) if c["gb"] else None,
            "g_x": Slot(dev, (B, K), f32, None, off.get("g_x", 0)) if c["gx"] else None}
    ops.dense_bwd(_t(ins["x"]), _t(ins["gy"]), _t(ins["w"]), g_w=_t(outs["g_w"]), g_b=_t(outs["g_b"]), g_x=_t(outs["g_x"]),
                  y=_t(ins["y"]), y_scale=c["y_scale"], gx_mask=c["mask"], gx_scale=c["gx_scale"], math_mode=_math(c, x3))
    torch.cuda.synchronize()
    for k, s in outs.items():
        assert s is None or s.intact(), (name, off, "a store outside " + k)
    for k in names:
        assert ins[k] is None or (ins[k].intact() and _same_bits(ins[k].t.cpu(), d[k])), (name, off, "an input changed")
    return tuple(_t(outs[k]) for k in R.BWD_NAMES)


@functools.lru_cache(maxsize=None)
def _bwd_aligned(dev, name):
    return _bwd(dev, name)


def _bwd_offsets(c):
    """Each operand and output whose row length is a multiple of 4, in turn one float past a 16-byte boundary."""
    out = []
    if c["K"] % 4 == 0:
        out += [{"x": 1}, {"w": 1}, {"g_w": 1}] + ([{"g_x": 1}] if c["gx"] else [])
    if c["N"] % 4 == 0:
        out += [{"gy": 1}] + ([{"y": 1}] if c["y"] else []) + ([{"g_b": 1}] if c["gb"] else [])
    return out


def _equal_outputs(a, b):
    return all((u is None and v is None) or _same_bits(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("name", list(R.BWD_CASES))
def test_backward_within_the_fp64_bound(dev, name):
    c, ref = R.BWD_CASES[name], R.bwd_reference(name)
    got = _bwd_aligned(dev, name)
    for n, g in zip(R.BWD_NAMES, got):
        assert g is None or not bool(torch.isnan(g).any()), f"an element of {n} was not written"
    sh = R.bwd_shares(got, ref)
    print(f"dense_bwd {c['math']:4s} {name:18s} share of the bound: "
          + "  ".join(f"{n} {s:.3f}" for n, s in zip(R.BWD_NAMES, sh) if s is not None))
    assert max(s for s in sh if s is not None) <= 1.0, (name, dict(zip(R.BWD_NAMES, sh)))
    for off in _bwd_offsets(c):
        assert _equal_outputs(_bwd(dev, name, off=off), got), (name, off, "misaligned run differs from the aligned run")


@pytest.mark.parametrize("name", [n for n, c in R.BWD_CASES.items() if c["math"] == "f32"])
def test_backward_bf16x3_equals_f32(dev, name):
    assert _equal_outputs(_bwd(dev, name, x3=True), _bwd_aligned(dev, name))


@pytest.mark.parametrize("name", [n for n, c in R.BWD_CASES.items() if c["gb"] and c["gx"]])
def test_optional_outputs_leave_the_others_bit_unchanged(dev, name):
    """g_x = None takes the g_x tiles off the front of the grid, so g_w and g_b come from other blocks: the same bits.
    g_b = None: g_w and g_x unchanged."""
    g_w, g_b, g_x = _bwd_aligned(dev, name)
    w1, b1, x1 = _bwd(dev, name, gx=False)
    assert x1 is None and _same_bits(w1, g_w) and _same_bits(b1, g_b)
    w2, b2, x2 = _bwd(dev, name, gb=False)
    assert b2 is None and _same_bits(w2, g_w) and _same_bits(x2, g_x)
    w3, b3, x3 = _bwd(dev, name, gb=False, gx=False)
    assert b3 is None and x3 is None and _same_bits(w3, g_w)
