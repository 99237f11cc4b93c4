"""CPU-side checks of the F9 pruning sweep (bnn_snr_select, bnn_prune_codes, bnn_pruned_fwd, bnn_prune_sweep_tail,
posthoc.PruneSweep; no GPU): the entry points exist, the ctypes mirrors match the header, every argument check runs on the
host before a launch, and the fp64 restatement the GPU tests compare against (thresholds, level codes, masked forward) --
kept in this file -- agrees with np.percentile and with the oracle's prune_weights."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import bnn_oracle as O
from test_bandit_cpu import _layout

FAKE = 0x10000
PAPER_LEVELS = (0., .5, .75, .95, .98)


# ------------------------------------------------------------------------------------------------- the fp64 restatement
def thresholds_ref(snrs, ps):
    """posthoc.snr_threshold for every p, in numpy: the fp32 SNRs as float64, sorted (NaNs last), the two order statistics
    around (n - 1) p, a + (b - a) (pos - lo), and a when a == b."""
    v = np.sort(np.asarray(snrs, dtype=np.float64).ravel())
    n = v.size
    out = []
    for p in ps:
        pos = (n - 1) * float(p)
        lo = int(np.floor(pos))
        hi = min(lo + 1, n - 1)
        a, b = float(v[lo]), float(v[hi])
        with np.errstate(invalid="ignore"):
            out.append(a if a == b else a + (b - a) * (pos - lo))
    return np.asarray(out, dtype=np.float64)


def codes_ref(snr32, thr_ascending):
    """code = #{p : snr > (float32) thr_p}: the comparison bnn_snr_prune makes, counted over the ascending thresholds."""
    s = np.asarray(snr32, dtype=np.float32)
    code = np.zeros(s.shape, dtype=np.uint8)
    for t in thr_ascending:
        with np.errstate(invalid="ignore"):
            code += (s > np.float32(t)).astype(np.uint8)
    return code


def _bf16(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).to(torch.bfloat16).double().numpy()


def masked_forward_ref(x, layers, level, bf16=False):
    """fp64 logits of the network pruned at `level`: layers = [(W [out, in], b [out], wcode, bcode)], ReLU between them;
    bf16: the operands rounded where the kernel rounds them (x, W and the hidden activations; the bias stays fp32), as
    tests/test_gpu_dense_train.py restates its bf16 forward."""
    h = np.asarray(x, dtype=np.float64).reshape(len(x), -1)
    for i, (W, b, wc, bc) in enumerate(layers):
        Wm = np.where(wc > level, W, 0.0).astype(np.float64)
        bm = np.where(bc > level, b, 0.0).astype(np.float64)
        if bf16:
            h, Wm = _bf16(h), _bf16(Wm)
        h = h @ Wm.T + bm
        if i + 1 < len(layers):
            h = np.maximum(h, 0.0)
    return h


def snr32_torch(mu, rho):
    """weight_pruning.py:98-102 in torch fp32 (the oracle's expressions)."""
    mu, rho = torch.as_tensor(mu), torch.as_tensor(rho)
    return (10 * torch.log10(torch.abs(mu) / torch.log1p(torch.exp(rho)))).numpy()


# ------------------------------------------------------------------------------------------------- exports and layouts
NEW = ("bnn_snr_select_workspace_bytes", "bnn_snr_select", "bnn_prune_codes", "bnn_pruned_fwd", "bnn_prune_sweep_tail")


def test_prune_sweep_exports():
    from bnn_hip import _lib as L, posthoc
    lib = L.load()
    assert lib.bnn_version() == L.ABI_VERSION
    for name in NEW:
        assert name in L.EXPORTS and hasattr(lib, name)
    assert lib.bnn_snr_select_workspace_bytes() >= 4 * 2 * L.PRUNE_MAX_LEVELS * 256
    assert callable(posthoc.snr_thresholds) and callable(posthoc.PruneSweep.evaluate) and callable(posthoc.PruneSweep.forward)


def test_prune_sweep_struct_layouts_match_the_header(tmp_path):
    from bnn_hip import _lib as L
    _layout(tmp_path, L.SnrSelectArgs, "bnn_snr_select_args",
            [("BNN_PRUNE_MAX_LEVELS", L.PRUNE_MAX_LEVELS), ("BNN_PRUNE_MAX_SEGMENTS", L.PRUNE_MAX_SEGMENTS),
             ("BNN_PRUNE_LEVELS_PER_LAUNCH", L.PRUNE_LEVELS_PER_LAUNCH), ("BNN_HIP_ABI_VERSION", L.ABI_VERSION)])
    _layout(tmp_path, L.PruneCodesArgs, "bnn_prune_codes_args")
    _layout(tmp_path, L.PrunedFwdArgs, "bnn_pruned_fwd_args")
    _layout(tmp_path, L.PruneTailArgs, "bnn_prune_tail_args")
    assert L.PRUNE_LEVELS_PER_LAUNCH == 8 and L.PRUNE_MAX_LEVELS == 16


# ------------------------------------------------------------------------------------------------- argument validation
def _select_args(**over):
    from bnn_hip import _lib as L
    a = L.SnrSelectArgs()
    a.struct_bytes = C.sizeof(L.SnrSelectArgs)
    a.n_segments, a.n_levels = 2, 3
    a.snr[0], a.snr[1], a.n[0], a.n[1] = FAKE, FAKE, 100, 7
    a.fraction[0], a.fraction[1], a.fraction[2] = 0.0, 0.5, 1.0
    a.workspace, a.workspace_bytes, a.thresholds = FAKE, L.load().bnn_snr_select_workspace_bytes(), FAKE
    for k, v in over.items():
        if isinstance(v, tuple):
            getattr(a, k)[v[0]] = v[1]
        else:
            setattr(a, k, v)
    return a


def test_select_argument_validation_without_a_device():
    """Fake, never dereferenced device addresses: every rejection happens before a launch."""
    from bnn_hip import _lib as L
    fn = L.load().bnn_snr_select
    assert fn(None, None) == -1                                                            # BNN_ERR_NULL
    assert fn(C.byref(_select_args(struct_bytes=C.sizeof(L.SnrSelectArgs) + 8)), None) == -5  # BNN_ERR_ABI
    for bad in (dict(n_segments=0), dict(n_segments=L.PRUNE_MAX_SEGMENTS + 1), dict(n_levels=0),
                dict(n_levels=L.PRUNE_MAX_LEVELS + 1), dict(n=(1, 0)), dict(n=(0, 1 << 31)), dict(n=(0, (1 << 31) - 7)),
                dict(fraction=(1, 1.5)), dict(fraction=(0, -0.1)), dict(fraction=(2, float("nan")))):
        assert fn(C.byref(_select_args(**bad)), None) == -2, bad                          # BNN_ERR_SHAPE
    assert fn(C.byref(_select_args(snr=(1, None))), None) == -1
    assert fn(C.byref(_select_args(thresholds=None)), None) == -1
    assert fn(C.byref(_select_args(workspace=None)), None) == -4                          # BNN_ERR_WORKSPACE
    assert fn(C.byref(_select_args(workspace_bytes=L.load().bnn_snr_select_workspace_bytes() - 1)), None) == -4
    assert fn(C.byref(_select_args(snr=(0, FAKE + 2))), None) == -6                       # BNN_ERR_ALIGN
    assert fn(C.byref(_select_args(thresholds=FAKE + 4)), None) == -6
    assert fn(C.byref(_select_args(workspace=FAKE + 4)), None) == -6


def _codes_args(**over):
    from bnn_hip import _lib as L
    a = L.PruneCodesArgs()
    a.struct_bytes = C.sizeof(L.PruneCodesArgs)
    a.out_features, a.in_features, a.ld, a.transposed, a.n_levels, a.mu_dtype = 10, 20, 32, 0, 5, L.F32
    for f in ("mu", "rho", "thresholds", "code", "mu_out", "kept"):
        setattr(a, f, FAKE)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_codes_argument_validation_without_a_device():
    from bnn_hip import _lib as L
    fn = L.load().bnn_prune_codes
    assert fn(None, None) == -1
    assert fn(C.byref(_codes_args(struct_bytes=4)), None) == -5
    for bad in (dict(out_features=0), dict(in_features=0), dict(ld=19), dict(n_levels=0), dict(n_levels=L.PRUNE_MAX_LEVELS + 1)):
        assert fn(C.byref(_codes_args(**bad)), None) == -2, bad
    for code in (2, -1):
        assert fn(C.byref(_codes_args(mu_dtype=code)), None) == -3, code                  # BNN_ERR_ENUM
    for f in ("mu", "rho", "thresholds", "code", "mu_out", "kept"):
        assert fn(C.byref(_codes_args(**{f: None})), None) == -1, f
    for f, off in (("mu", 2), ("rho", 1), ("thresholds", 4), ("kept", 4), ("mu_out", 2)):
        assert fn(C.byref(_codes_args(**{f: FAKE + off})), None) == -6, f
    assert fn(C.byref(_codes_args(mu_out=FAKE + 1, mu_dtype=L.BF16)), None) == -6


def _fwd_args(**over):
    from bnn_hip import _lib as L
    a = L.PrunedFwdArgs()
    a.struct_bytes = C.sizeof(L.PrunedFwdArgs)
    a.n_levels, a.rows, a.in_features, a.out_features, a.math, a.relu, a.x_shared = 5, 37, 100, 10, L.MATH_F32, 1, 1
    a.x_dtype, a.y_dtype, a.ldx, a.ldy, a.ld = L.F32, L.F32, 100, 10, 128
    for f in ("x", "mu", "code", "b", "bcode", "y"):
        setattr(a, f, FAKE)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_forward_argument_validation_without_a_device():
    from bnn_hip import _lib as L
    fn = L.load().bnn_pruned_fwd
    assert fn(None, None) == -1
    assert fn(C.byref(_fwd_args(struct_bytes=C.sizeof(L.PrunedFwdArgs) - 4)), None) == -5
    for bad in (dict(n_levels=0), dict(n_levels=L.PRUNE_MAX_LEVELS + 1), dict(rows=0), dict(in_features=0), dict(out_features=-1),
                dict(ld=100), dict(ld=96), dict(ldx=99), dict(ldy=9)):
        assert fn(C.byref(_fwd_args(**bad)), None) == -2, bad
    for bad in (dict(math=3), dict(math=-1), dict(x_dtype=2), dict(y_dtype=7), dict(x_dtype=L.BF16), dict(y_dtype=L.BF16),
                dict(math=L.MATH_BF16), dict(math=L.MATH_BF16X3, x_dtype=L.BF16)):
        assert fn(C.byref(_fwd_args(**bad)), None) == -3, bad                             # a dtype the math mode does not take
    for f in ("x", "mu", "code", "y", "b", "bcode"):
        assert fn(C.byref(_fwd_args(**{f: None})), None) == -1, f                         # (b and bcode: both or neither)
    for f, off in (("mu", 8), ("code", 4), ("x", 2), ("y", 2), ("b", 2)):
        assert fn(C.byref(_fwd_args(**{f: FAKE + off})), None) == -6, f
    assert fn(C.byref(_fwd_args(math=L.MATH_BF16, x_dtype=L.BF16, y_dtype=L.BF16, x=FAKE + 1)), None) == -6


def _tail_args(**over):
    from bnn_hip import _lib as L
    a = L.PruneTailArgs()
    a.struct_bytes = C.sizeof(L.PruneTailArgs)
    a.mode, a.n_levels, a.rows, a.classes, a.n_total, a.row0 = L.NLL_CLASSIFICATION, 5, 128, 10, 1000, 256
    for f in ("logits", "target", "probs", "correct", "loss"):
        setattr(a, f, FAKE)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_tail_argument_validation_without_a_device():
    from bnn_hip import _lib as L
    fn = L.load().bnn_prune_sweep_tail
    assert fn(None, None) == -1
    assert fn(C.byref(_tail_args(struct_bytes=0)), None) == -5
    for code in (2, -1):
        assert fn(C.byref(_tail_args(mode=code)), None) == -3, code
    for bad in (dict(n_levels=0), dict(n_levels=17), dict(rows=0), dict(classes=0), dict(row0=-1), dict(row0=900), dict(n_total=0)):
        assert fn(C.byref(_tail_args(**bad)), None) == -2, bad
    for f in ("logits", "target", "probs", "correct", "loss"):
        assert fn(C.byref(_tail_args(**{f: None})), None) == -1, f
    for f in ("logits", "target", "loss"):                                                # regression needs no probs / correct
        assert fn(C.byref(_tail_args(mode=L.NLL_REGRESSION, probs=None, correct=None, **{f: None})), None) == -1, f
    for f, off in (("logits", 2), ("target", 4), ("probs", 2), ("correct", 4), ("loss", 4)):
        assert fn(C.byref(_tail_args(**{f: FAKE + off})), None) == -6, f
    assert fn(C.byref(_tail_args(mode=L.NLL_REGRESSION, target=FAKE + 2)), None) == -6


def test_host_api_rejects_what_cannot_run():
    from bnn_hip import posthoc
    from bnn_hip.ops import BnnHipError
    with pytest.raises(BnnHipError, match="no CPU fallback"):
        posthoc.snr_thresholds(torch.zeros(8), (0.5,))
    with pytest.raises(BnnHipError, match="drop fractions"):
        posthoc.PruneSweep(torch.nn.Linear(2, 2), drop_percentages=(1.5,))
    with pytest.raises(BnnHipError, match="drop fractions"):
        posthoc.PruneSweep(torch.nn.Linear(2, 2), drop_percentages=tuple([0.5] * 17))


# ------------------------------------------------------------------------------------------------- the restatement itself
@pytest.mark.parametrize("n,seed", [(1, 0), (2, 1), (190, 2), (4097, 3), (100003, 4)])
def test_threshold_restatement_agrees_with_numpy_percentile(n, seed):
    """Both are fp64 linear interpolations between the same two order statistics of values below ~10^3 in magnitude: they
    differ by a few ulps of the values at most, far inside 1e-12 absolute."""
    rs = np.random.RandomState(seed)
    snr = (rs.standard_normal(n) * 12 + 5).astype(np.float32)
    if n > 100:
        snr[rs.randint(0, n, n // 3)] = snr[0]                      # heavy ties
    ps = (0, .25, .5, .75, .95, .98, 1)
    got = thresholds_ref(snr, ps)
    want = np.asarray([np.percentile(snr.astype(np.float64), 100 * p) for p in ps])
    assert np.abs(got - want).max() <= 1e-12
    assert np.all(np.diff(got) >= 0)


def test_restated_masks_equal_the_oracle_prune_weights_survivors():
    rs = np.random.RandomState(9)
    layer = tuple(torch.from_numpy(a.astype(np.float32)) for a in (rs.uniform(-0.2, 0.2, (24, 17)), rs.uniform(-5, -4, (24, 17)),
                                                                    rs.uniform(-0.2, 0.2, 24), rs.uniform(-5, -4, 24)))
    layer[0].view(-1)[5] = 0.0                                       # -inf dB
    snr_w, snr_b = snr32_torch(layer[0], layer[1]), snr32_torch(layer[2], layer[3])
    allsnr = np.concatenate([snr_w.ravel(), snr_b.ravel()])
    levels = (0.25, .5, .75, .95, .98)                              # (finite order statistics: the oracle's np.percentile agrees)
    thr = thresholds_ref(allsnr, levels)
    wc, bc = codes_ref(snr_w, thr), codes_ref(snr_b, thr)
    for i, p in enumerate(levels):
        pruned, thr_o = O.prune_weights([layer], allsnr.astype(np.float64), p)
        wm, _, bm, _ = pruned[0]
        assert abs(thr_o - thr[i]) <= 1e-12
        assert np.array_equal(wc > i, (wm != 0).numpy()) and np.array_equal(bc > i, (bm != 0).numpy())
    assert wc.ravel()[5] == 0 and wc.max() == len(levels)


def test_masked_forward_restatement_levels():
    """Level codes are nested: a level's survivors contain the next level's, and a code of P survives every level."""
    rs = np.random.RandomState(3)
    W, b = rs.uniform(-1, 1, (6, 4)), rs.uniform(-1, 1, 6)
    wc, bc = rs.randint(0, 4, (6, 4)).astype(np.uint8), rs.randint(0, 4, 6).astype(np.uint8)
    x = rs.uniform(0, 1, (5, 4))
    full = masked_forward_ref(x, [(W, b, wc + 10, bc + 10)], 0)
    np.testing.assert_allclose(full, x @ W.T + b, rtol=1e-15)
    assert np.array_equal(masked_forward_ref(x, [(W, b, wc, bc)], 3), np.zeros((5, 6)))
    one = masked_forward_ref(x, [(W, b, wc, bc)], 1)
    np.testing.assert_allclose(one, x @ np.where(wc > 1, W, 0).T + np.where(bc > 1, b, 0), rtol=1e-15)
