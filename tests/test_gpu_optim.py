"""The fused optimiser steps (bnn_adam_step: csrc/optim.hip; bnn_sgd_step: csrc/dense_train.hip; the wrappers of
bnn_hip/optim.py) on an MI355X against the fp64 restatement tests/optim_ref.py: EVERY element of p', m', v' under its own
derived bound (the derivation is that module's docstring; tests/test_optim_cpu.py proves the restatement against
torch.optim, the bound wide enough for the kernels' fp32 arithmetic and tight enough for seeded wrong variants), every
launch form against the host-step launch bit for bit, the ticketed hand-off at every grid around its group boundaries, and
every tensor between guard bands.

Nothing was tuned on the device's figures; measured afterwards (largest |got - ref| / bound over all elements of all cases
of a family; beside it the fp32 emulation's figure from tests/test_optim_cpu.py, which needs no device):
                         device                       emulation
                         p'       m'       v'         p'     m'     v'
  regimes, fp32 g        0.99688  0.99856  0.73611    0.997  0.999  0.736
  regimes, bf16 g        0.99596  0.99985  0.75670    0.996  1.000  0.757
  geometry, fp32 g       0.98948  0.99371  0.73960    0.989  0.994  0.740
  geometry, bf16 g       0.99709  0.98293  0.73415    0.997  0.983  0.734
  SGD                    0.99490                      0.995
  FusedAdam, 12 steps    0.99493  0.92562  0.81299    (capturable: 0.99500  0.92562  0.81299)
  FusedSGD, 12 steps     0.99693                      (capturable: 0.99680)
p' is set by its own final half-ulp rounding, m' by the final rounding of an m' just above a power of two whose gg - m is
small (the emulation's 1.000 is 0.99985, the same element); the device and the emulation agree to the digits shown.
"""
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import optim_ref as R
from bnn_hip import ops
from bnn_hip.optim import FusedAdam, FusedSGD


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


class Call:
    """A call's tensors on the device: per kind (p, g, m, v) one buffer, every tensor a 16-byte-aligned view between guard
    bands of 64 sentinel floats (optim_ref.arena)."""

    def __init__(self, tensors, dev, keys="pgmv", bf16=False):
        self.keys, self.spans, self.buf, self.views, self.g_in = keys, {}, {}, {}, [t["g"] for t in tensors]
        for k in keys:
            half = bf16 and k == "g"
            image, self.spans[k] = R.arena([t[k] for t in tensors], 2 if half else 4)
            self.buf[k] = torch.from_numpy(image.view(np.int16 if half else np.int32)).to(dev)
            typed = self.buf[k].view(torch.bfloat16 if half else torch.float32)
            self.views[k] = [typed[o:o + n] for o, n in self.spans[k]]
            assert all(v.data_ptr() % 16 == 0 and v.is_contiguous() for v in self.views[k])

    def read(self):
        """Per kind the tensors as numpy float32 (bf16 widened); asserts the guard bands and that g is unchanged in bits."""
        out = {}
        for k in self.keys:
            image = self.buf[k].cpu().numpy()
            image = image.view(np.uint16 if image.dtype == np.int16 else np.uint32)
            assert R.arena_guards_intact(image, self.spans[k]), f"a write outside the tensors of {k}"
            wide = (image.astype(np.uint32) << 16) if image.dtype == np.uint16 else image
            out[k] = [wide[o:o + n].view(np.float32) for o, n in self.spans[k]]
        for a, b in zip(out["g"], self.g_in):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "the gradient was written"
        return out

    def outputs(self):
        r = self.read()
        return [tuple(r[k][i] for k in "pmv") for i in range(len(self.g_in))]


def _word(value, dev):
    """A uint32 device word (torch holds it as int32)."""
    return torch.tensor([value - 2 ** 32 if value >= 2 ** 31 else value], dtype=torch.int32, device=dev)


def _u32(word):
    return int(word) % 2 ** 32


def _adam(call, c, dev, *, step_form="host", lr_device=False, lr=None, words=None):
    """One ops.adam_step call over `call`.  step_form: 'host' (step by argument), 'tick' (device word, advanced by the tick
    launch), 'ticket' (device word, advanced by the update launch's last block).  Returns the device words used."""
    lr = c["lr"] if lr is None else lr
    kw = dict(lr=lr, betas=(c["b1"], c["b2"]), eps=c["eps"], weight_decay=c["wd"])
    words = dict(words or {})
    if lr_device:
        words.setdefault("lr", torch.tensor([lr], dtype=torch.float32, device=dev))
        kw.update(lr=123.0, lr_device=words["lr"])                    # the argument must be ignored
    if step_form == "host":
        kw["step"] = c["step"]
    else:
        words.setdefault("step", _word(c["step"] - 1, dev))
        kw["step_device"] = words["step"]
        if step_form == "ticket":
            words.setdefault("ticket", torch.zeros(16, dtype=torch.int32, device=dev))
            kw["ticket"] = words["ticket"]
            if "bump" in words:
                kw.update(bump_counter=words["bump"], bump_by=words["bump_by"])
    v = call.views
    ops.adam_step(v["p"], v["g"], v["m"], v["v"], **kw)
    return words


def _bits_equal(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for ta, tb in zip(a, b) for x, y in zip(ta, tb))


def _fmt(sh):
    return "  ".join(f"{k}' {s:.5f}" for k, s in sh.items())


# ------------------------------------------------------------------------------------------ one launch against the bound
@pytest.mark.parametrize("gdtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(R.ADAM_CASES))
def test_adam_step_within_the_fp64_bound(dev, name, gdtype):
    """Every element of p', m', v' of every case (the regimes of one 4099-element tensor; the geometry calls of 16 and 19
    tensors and the grids of 1 .. 17 chunks), guard bands intact, g untouched."""
    bf16 = gdtype == "bf16"
    c = R.ADAM_CASES[name]
    call = Call(R.adam_inputs(name, bf16), dev, bf16=bf16)
    _adam(call, c, dev)
    sh = R.adam_shares(call.outputs(), R.adam_expected(name, bf16))
    print(f"{name:36s} {gdtype} g  share of the bound: {_fmt(sh)}")
    assert max(sh.values()) <= 1.0, (name, gdtype, sh)


# ------------------------------------------------------------------------------------------ launch forms, bit for bit
FORM_CASES = ("s7-wd0.01-eps1e-08-b0.9_0.999", "s1-wd0-eps0.001-b0_0.999", "s4294967295-wd0-eps1e-08-b0.9_0.999", "geo16", "geo19")


@pytest.mark.parametrize("name", FORM_CASES)
def test_launch_forms_agree_bit_for_bit(dev, name):
    """Host step; device step with the tick launch; device step with the ticket; each with the learning rate in a device
    word; each with bf16 gradients against the same values widened to fp32: the bits of the host-step fp32 launch."""
    c = R.ADAM_CASES[name]
    tensors = R.adam_inputs(name, True)                               # bf16 values, as fp32 arrays
    base = Call(tensors, dev)
    _adam(base, c, dev, lr=R.LR32)
    want = base.outputs()
    for bf16 in (False, True):
        for step_form in ("host", "tick", "ticket"):
            for lr_device in (False, True):
                call = Call(tensors, dev, bf16=bf16)
                words = _adam(call, c, dev, step_form=step_form, lr_device=lr_device, lr=R.LR32)
                what = (name, "bf16" if bf16 else "fp32", step_form, "lr word" if lr_device else "lr argument")
                assert _bits_equal(call.outputs(), want), what
                if step_form != "host":
                    assert _u32(words["step"]) == c["step"], what
                if step_form == "ticket":
                    assert int(words["ticket"].abs().sum()) == 0, what


@pytest.mark.parametrize("gdtype", ["fp32", "bf16"])
def test_whole_chunk_body_and_general_loop_agree_bit_for_bit(dev, gdtype):
    """The same values as a 4096-element tensor (the whole-chunk body), as the first chunk of a 4099-element tensor, and as
    tensors of 4095 and 4092 elements (the general loop: ragged, and ending on a full group of four)."""
    bf16 = gdtype == "bf16"
    name = "s7-wd0.01-eps1e-08-b0.9_0.999"
    c = R.ADAM_CASES[name]
    (t,) = R.adam_inputs(name, bf16)
    cut = lambda n: {k: a[:n] for k, a in t.items()}
    got = {}
    for n in (4099, 4096, 4095, 4092, 5):
        call = Call([cut(n)], dev, bf16=bf16)
        _adam(call, c, dev)
        (got[n],) = call.outputs()
    assert [R.block_kind((n,), R.chunk_table((n,))[0]) for n in (4099, 4096, 4095, 4092)] == ["whole", "whole", "ragged", "full4"]
    for n in (4096, 4095, 4092, 5):
        assert _bits_equal([tuple(a[:n] for a in got[4099])], [got[n]]), n


# ------------------------------------------------------------------------------------------ the ticketed hand-off
@pytest.mark.parametrize("grid", list(R.GRIDS))
def test_ticketed_hand_off_at_every_grid(dev, grid):
    """Three launches of exactly `grid` blocks (the two-level arrival count: fewer than 8 groups, 8, one group of two):
    the step word advances by exactly 1 per launch, the bump word by bump_by, all 16 ticket words end at zero, and every
    block used the same step -- the outputs are the host-step launch's bits."""
    name = f"grid{grid}"
    c = dict(R.ADAM_CASES[name])
    tensors = R.adam_inputs(name)
    assert len(R.chunk_table(c["sizes"])) == grid
    a, b = Call(tensors, dev), Call(tensors, dev)
    words = dict(step=_word(c["step"] - 1, dev), ticket=torch.zeros(16, dtype=torch.int32, device=dev), bump=_word(100, dev),
                 bump_by=5)
    for k in range(3):
        _adam(a, c, dev, step_form="ticket", words=words)
        _adam(b, dict(c, step=c["step"] + k), dev)
        assert _u32(words["step"]) == c["step"] + k, (grid, k)
        assert words["ticket"].cpu().tolist() == [0] * 16, (grid, k)
        assert _u32(words["bump"]) == 100 + 5 * (k + 1), (grid, k)
        assert _bits_equal(a.outputs(), b.outputs()), (grid, k)


# ------------------------------------------------------------------------------------------ SGD
def _sgd(call, c, dev, lr, lr_device):
    kw = dict(lr=lr, weight_decay=c["wd"])
    if lr_device:
        kw.update(lr=123.0, lr_device=torch.tensor([lr], dtype=torch.float32, device=dev))
    ops.sgd_step(call.views["p"], call.views["g"], **kw)


@pytest.mark.parametrize("name", list(R.SGD_CASES))
def test_sgd_step_within_the_fp64_bound(dev, name):
    """The regime tensor, the 16-tensor launch and a 17-tensor call (two launches), lr by argument and from a device word
    (the same bits), guard bands intact, g untouched."""
    c = R.SGD_CASES[name]
    got = {}
    for lr_device in (False, True):
        call = Call(R.sgd_inputs(name), dev, keys="pg")
        _sgd(call, c, dev, c["lr"], lr_device)
        got[lr_device] = call.read()["p"]
        lr_used = float(np.float32(c["lr"])) if lr_device else c["lr"]
        sh = R.sgd_share(got[lr_device], R.sgd_expected(name, lr_used))
        print(f"{name:24s} lr {'word' if lr_device else 'argument'}  share of the bound: p' {sh:.5f}")
        assert sh <= 1.0, (name, lr_device, sh)
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(got[False], got[True]))


@pytest.mark.parametrize("lr_device", [False, True])
def test_sgd_step_with_lr_zero_leaves_p_unchanged_in_bits(dev, lr_device):
    name = "sgd-geo17-wd0.001"
    tensors = R.sgd_inputs(name)
    call = Call(tensors, dev, keys="pg")
    _sgd(call, R.SGD_CASES[name], dev, 0.0, lr_device)
    for a, t in zip(call.read()["p"], tensors):
        assert np.array_equal(a.view(np.uint32), t["p"].view(np.uint32))


# ------------------------------------------------------------------------------------------ the wrappers, step by step
WRAP_SIZES = (5000, 9, 4096, 33)
WRAP_STEPS, WRAP_LR = 12, 2e-3


def _params(rs, dev):
    return [torch.nn.Parameter(torch.from_numpy(rs.standard_normal(n).astype(np.float32)).to(dev)) for n in WRAP_SIZES]


def _grads(rs, ps):
    gs = [(rs.standard_normal(p.numel()) * 10.0 ** rs.randint(-4, 2)).astype(np.float32) for p in ps]
    for p, g in zip(ps, gs):
        p.grad = torch.from_numpy(g).to(p.device)
    return gs


def _np(t):
    return t.detach().cpu().numpy().copy()


@pytest.mark.parametrize("capturable", [False, True])
def test_fused_adam_under_steplr_step_by_step(dev, capturable):
    """12 steps under StepLR(3, 0.5): after each, p and state[p] against the ONE-step restatement from the values read back
    before it -- the bound, no drift tolerance.  After step 6 the state goes through state_dict() / load_state_dict() into
    a fresh capturable optimiser, whose next step must be step 7, not 1."""
    rs = np.random.RandomState(zlib.crc32(b"fused-adam-wrapper") & 0x7FFFFFFF)
    kw = dict(lr=WRAP_LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    ps = _params(rs, dev)
    opt = FusedAdam(ps, capturable=capturable, **kw)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=3, gamma=0.5)
    worst = dict.fromkeys(R.NAMES, 0.0)
    for step in range(1, WRAP_STEPS + 1):
        cap = opt.param_groups[0]["capturable"]
        lr = opt.param_groups[0]["lr"]
        assert abs(lr - WRAP_LR * 0.5 ** ((step - 1) // 3)) <= 1e-12 * lr
        before = []
        for p in ps:
            st = opt.state.get(p, {})
            zero = np.zeros(p.numel(), dtype=np.float32)
            before.append((_np(p), _np(st["exp_avg"]) if "exp_avg" in st else zero, _np(st["exp_avg_sq"]) if "exp_avg_sq" in st else zero))
        gs = _grads(rs, ps)
        opt.step()
        lr_used = float(np.float32(lr)) if cap else lr                 # a capturable group reads its fp32 device word
        expected = [R.adam_ref(p0, g, m0, v0, lr=lr_used, b1=0.9, b2=0.999, eps=1e-8, wd=0.01, step=step)
                    for (p0, m0, v0), g in zip(before, gs)]
        got = [(_np(p), _np(opt.state[p]["exp_avg"]), _np(opt.state[p]["exp_avg_sq"])) for p in ps]
        sh = R.adam_shares(got, expected)
        assert max(sh.values()) <= 1.0, (step, sh)
        worst = {k: max(worst[k], sh[k]) for k in worst}
        if cap:
            assert opt.device_step() == step
        else:
            assert all(int(opt.state[p]["step"]) == step for p in ps)
        sched.step()
        if step == WRAP_STEPS // 2:
            sd = opt.state_dict()
            assert all(int(s["step"]) == step for s in sd["state"].values())
            ps2 = [torch.nn.Parameter(p.detach().clone()) for p in ps]
            opt2 = FusedAdam(ps2, capturable=True, **kw)
            opt2.load_state_dict(sd)
            sched2 = torch.optim.lr_scheduler.StepLR(opt2, step_size=3, gamma=0.5)
            sched2.load_state_dict(sched.state_dict())
            ps, opt, sched = ps2, opt2, sched2
    print(f"FusedAdam {'capturable' if capturable else 'plain':10s} 12 steps  share of the bound: {_fmt(worst)}")


@pytest.mark.parametrize("capturable", [False, True])
def test_fused_sgd_under_steplr_step_by_step(dev, capturable):
    rs = np.random.RandomState(zlib.crc32(b"fused-sgd-wrapper") & 0x7FFFFFFF)
    ps = _params(rs, dev)
    opt = FusedSGD(ps, lr=0.05, weight_decay=1e-3, capturable=capturable)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=3, gamma=0.5)
    worst = 0.0
    for step in range(1, WRAP_STEPS + 1):
        lr = opt.param_groups[0]["lr"]
        assert abs(lr - 0.05 * 0.5 ** ((step - 1) // 3)) <= 1e-12 * lr
        before = [_np(p) for p in ps]
        gs = _grads(rs, ps)
        opt.step()
        lr_used = float(np.float32(lr)) if capturable else lr
        sh = R.sgd_share([_np(p) for p in ps], [R.sgd_ref(p0, g, lr=lr_used, wd=1e-3) for p0, g in zip(before, gs)])
        assert sh <= 1.0, (step, sh)
        worst = max(worst, sh)
        sched.step()
    print(f"FusedSGD  {'capturable' if capturable else 'plain':10s} 12 steps  share of the bound: p' {worst:.5f}")
