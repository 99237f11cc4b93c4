"""CPU-side checks of SG-MCMC and the weight bank (bnn_sgmcmc_noise, bnn_sgmcmc_step, bnn_bank_fwd, bnn_hip.sgmcmc;
include/bnn_hip.h F19; no GPU): the entry points exist and the ABI version is unchanged, the ctypes mirrors match the header,
malformed arguments are refused on the host in the documented order, the host's table builder agrees with the fp64 formulas, and
the numpy restatement (tests/sgmcmc_ref.py) is checked on its own: the stream against the oracle's generator, the exact fma, the
ring, the layout, and the stationary law of the update rule on the two chains the GPU test runs through the kernel."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import sgmcmc_ref as R
from test_bandit_cpu import _layout
from test_laplace_cpu import ABI, ALIGN, ENUM, FAKE, NULL, SHAPE, _args, _merge, _refused

NEW = ("bnn_sgmcmc_noise", "bnn_sgmcmc_step", "bnn_bank_fwd")
SEED = 0x5EED0123456789AB


def _L():
    from bnn_hip import _lib as L
    return L


def test_sgmcmc_exports_and_abi_version():
    L = _L()
    lib = L.load()
    assert lib.bnn_version() == 9 == L.ABI_VERSION
    for name in NEW:
        assert name in L.EXPORTS and hasattr(lib, name)
    import bnn_hip
    import networks
    from bnn_hip import ops, sgmcmc
    assert bnn_hip.FusedSGMCMC is sgmcmc.FusedSGMCMC and bnn_hip.WeightBank is sgmcmc.WeightBank
    for name in ("sgmcmc_noise", "sgmcmc_step", "bank_fwd", "bank_layout"):
        assert callable(getattr(ops, name))
    for name in ("views", "push", "member", "count", "state_dict", "load_state_dict", "forward", "predict_mc", "predictive", "score",
                 "evaluate", "predictive_graph"):
        assert callable(getattr(sgmcmc.WeightBank, name))
    assert callable(networks.MLP.sgmcmc) and callable(networks.MLP.weight_bank) and callable(networks.MLP_Dropout.sgmcmc)
    header = open(_layout.__globals__["HEADER"]).read()
    assert "int bnn_sgmcmc_noise(float* out, uint64_t seed, uint32_t tensor, uint32_t step, int64_t numel, void* stream);" in header
    assert "int bnn_sgmcmc_step(const bnn_sgmcmc_args* args, void* stream);" in header
    assert "int bnn_bank_fwd(const bnn_bank_fwd_args* args, void* stream);" in header
    assert "F19" in header and "#define BNN_HIP_ABI_VERSION 9" in header and "#define BNN_EPS_MAP_VERSION 2" in header


def test_sgmcmc_struct_layouts_match_the_header(tmp_path):
    L = _L()
    _layout(tmp_path, L.SgmcmcArgs, "bnn_sgmcmc_args",
            [("BNN_SGMCMC_MAX_TENSORS", L.SGMCMC_MAX_TENSORS), ("BNN_SGMCMC_TABLE_COLS", L.SGMCMC_TABLE_COLS),
             ("BNN_EPS_PHILOX", L.EPS_PHILOX), ("BNN_EPS_MEMORY", L.EPS_MEMORY), ("BNN_EPS_ZERO", L.EPS_ZERO),
             ("BNN_HIP_ABI_VERSION", L.ABI_VERSION)])
    _layout(tmp_path, L.BankFwdArgs, "bnn_bank_fwd_args")
    assert L.SGMCMC_MAX_TENSORS == R.MAX_TENSORS == 16


# ---------------------------------------------------------------------------------------------- the documented error order
def _step(**over):
    L = _L()
    two = {0: FAKE, 1: FAKE}
    d = dict(n_tensors=2, param=two, grad=two, momentum=two, noise=two, numel={0: 5000, 1: 7}, grad_scale=468.75, tau=0.5,
             eps_mode=L.EPS_MEMORY, table_rows=3, seed=7, burn_in=2, capacity=4)
    return _args(L.SgmcmcArgs, ("table", "step", "collected", "ticket", "bank"), **_merge(d, over))


def _bank(**over):
    L = _L()
    d = dict(members=3, first=1, batch=5, in_features=37, out_features=10, x_shared=1, relu=1, x_dtype=L.F32, math=L.MATH_F32,
             w_stride=448, b_stride=448, y_dtype=L.F32)
    return _args(L.BankFwdArgs, ("x", "w", "b", "y"), **dict(d, **over))


def test_sgmcmc_step_argument_errors():
    L = _L()
    fn = L.load().bnn_sgmcmc_step
    _refused(fn, _step, C.sizeof(L.SgmcmcArgs), [
        (SHAPE, (dict(n_tensors=0), dict(n_tensors=-1), dict(n_tensors=L.SGMCMC_MAX_TENSORS + 1), dict(table_rows=0),
                 dict(capacity=0), dict(capacity=-3), dict(numel={1: 0}), dict(numel={0: -5}), dict(numel={0: (1 << 34) + 1}))),
        (ENUM, (dict(eps_mode=3), dict(eps_mode=-1))),
        (NULL, (dict(table=None), dict(step=None), dict(ticket=None), dict(collected=None), dict(param={1: None}),
                dict(grad={0: None}), dict(momentum={1: None}), dict(momentum={0: None}), dict(noise={1: None}))),
        (ALIGN, (dict(param={0: FAKE + 4}), dict(grad={1: FAKE + 8}), dict(momentum={0: FAKE + 4, 1: FAKE + 4}),
                 dict(noise={0: FAKE + 4}), dict(table=FAKE + 4), dict(bank=FAKE + 8), dict(step=FAKE + 2),
                 dict(collected=FAKE + 1), dict(ticket=FAKE + 2))),
    ])
    # what a mode does not need may be NULL: no bank -> capacity and collected unread; no momentum at all; noise off MEMORY
    assert fn(C.byref(_step(bank=None, capacity=0, collected=None, param={0: None})), None) == NULL
    assert fn(C.byref(_step(momentum={0: None, 1: None}, eps_mode=L.EPS_ZERO, noise={0: None, 1: None}, table=None)), None) == NULL
    assert fn(C.byref(_step(momentum={0: None, 1: None}, eps_mode=L.EPS_PHILOX, noise={0: None, 1: None}, table=FAKE + 4)), None) == ALIGN
    # shape before enum, enum before NULL, NULL before alignment
    assert fn(C.byref(_step(table_rows=0, eps_mode=9, table=None)), None) == SHAPE
    assert fn(C.byref(_step(eps_mode=9, table=None, step=FAKE + 2)), None) == ENUM
    assert fn(C.byref(_step(table=None, step=FAKE + 2)), None) == NULL


def test_bank_fwd_argument_errors():
    L = _L()
    fn = L.load().bnn_bank_fwd
    _refused(fn, _bank, C.sizeof(L.BankFwdArgs), [
        (SHAPE, (dict(members=0), dict(first=-1), dict(batch=0), dict(in_features=0), dict(out_features=-2), dict(w_stride=-1),
                 dict(b_stride=-1), dict(members=1 << 20, batch=1 << 20, out_features=64))),
        (ENUM, (dict(math=3), dict(math=-1), dict(x_dtype=2), dict(y_dtype=-1), dict(x_dtype=L.BF16), dict(y_dtype=L.BF16),
                dict(math=L.MATH_BF16X3, y_dtype=L.BF16))),
        (NULL, (dict(x=None), dict(w=None), dict(y=None))),
        (ALIGN, (dict(x=FAKE + 2), dict(w=FAKE + 1), dict(b=FAKE + 2), dict(y=FAKE + 3),
                 dict(math=L.MATH_BF16, x_dtype=L.BF16, x=FAKE + 1))),
    ])
    assert fn(C.byref(_bank(batch=0, math=9, x=None)), None) == SHAPE
    assert fn(C.byref(_bank(math=9, x=None, y=FAKE + 1)), None) == ENUM
    assert fn(C.byref(_bank(x=None, y=FAKE + 1)), None) == NULL
    assert fn(C.byref(_bank(b=None, y=FAKE + 1)), None) == ALIGN                # (no bias is not an error)
    assert fn(C.byref(_bank(math=L.MATH_BF16, x_dtype=L.BF16, y_dtype=L.BF16, x=FAKE + 2, y=None)), None) == NULL


def test_sgmcmc_noise_argument_errors():
    fn = _L().load().bnn_sgmcmc_noise
    assert fn(None, 1, 0, 0, 8, None) == NULL
    assert fn(FAKE, 1, 0, 0, 0, None) == SHAPE and fn(FAKE, 1, 16, 0, 8, None) == SHAPE and fn(FAKE, 1, 0, 0, (1 << 34) + 1, None) == SHAPE
    assert fn(FAKE + 2, 1, 15, 0xFFFFFFFF, 8, None) == ALIGN


def test_host_side_refusals():
    import networks
    from bnn_hip import ops, sgmcmc
    from bnn_hip.ops import BnnHipError
    mp = dict(input_shape=5, classes=3, batch_size=4, hidden_units=6, mode="classification")
    with pytest.raises(BnnHipError):                              # CPU parameters: no fallback
        networks.MLP(mp).weight_bank(3)
    with pytest.raises(BnnHipError):
        ops.sgmcmc_noise(1, 0, 0, 8, "cpu")
    with pytest.raises(BnnHipError):
        ops.bank_fwd(torch.zeros(4, 5), torch.zeros(2, 64), 0, None, out_features=3, members=2)
    with pytest.raises(BnnHipError):
        ops.sgmcmc_step([torch.zeros(4)], [torch.zeros(4)], table=torch.zeros(1, 4), step=torch.zeros(1, dtype=torch.int32),
                        ticket=torch.zeros(16, dtype=torch.int32), grad_scale=1.0, tau=1.0)
    p = [torch.nn.Parameter(torch.zeros(4))]
    for bad in (dict(lr=0.0), dict(thin=0), dict(cycle_length=0), dict(collect_fraction=0.0), dict(collect_fraction=1.5),
                dict(friction=0.0), dict(friction=1.5), dict(burn_in=-1), dict(dataset_size=0)):
        with pytest.raises(ValueError):
            sgmcmc.FusedSGMCMC(p, **dict(dict(lr=0.1, dataset_size=10, batch_size=2), **bad))
    opt = sgmcmc.FusedSGMCMC(p, 0.1, dataset_size=60000, batch_size=128, friction=0.1, capturable=False)
    assert opt.grad_scale == 468.75 and opt._dev == {} and opt.device_step() == 0
    assert opt.param_groups[0]["capturable"] is False and opt.param_groups[0]["friction"] == 0.1


# ---------------------------------------------------------------------------------------------- the table builder
@pytest.mark.parametrize("friction", [None, 0.3])
def test_table_rows_are_the_fp64_formulas_rounded_once(friction):
    from bnn_hip import sgmcmc
    lr, T = 0.0123, 0.7
    t = sgmcmc.build_table(lr, temperature=T, friction=friction, thin=3)
    assert t.dtype == np.float32 and t.shape == (3, 4) and (t[0] == t[1]).all() and list(t[:, 3]) == [0, 0, 1]
    if friction is None:
        want = [lr / 2, 0.0, math.sqrt(lr * T)]
    else:
        want = [lr, 1 - friction, math.sqrt(2 * friction * lr * T)]
    assert [float(v) for v in t[0, :3]] == [float(np.float32(v)) for v in want]
    assert np.array_equal(t, R.table(R.learning_rates(lr, 3), T, friction, [0, 0, 1]))
    # the cyclical schedule
    Lc = 20
    c = sgmcmc.build_table(lr, temperature=T, friction=friction, thin=2, cycle_length=Lc, collect_fraction=0.25)
    lrs = [lr / 2 * (math.cos(math.pi * j / Lc) + 1) for j in range(Lc)]
    np.testing.assert_allclose(sgmcmc.learning_rates(lr, 2, Lc), lrs, rtol=1e-12)
    assert lrs[0] == lr and 0 < lrs[-1] < lr * 0.01
    for j in range(Lc):
        a = lrs[j] / 2 if friction is None else lrs[j]
        cc = math.sqrt(lrs[j] * T) if friction is None else math.sqrt(2 * friction * lrs[j] * T)
        assert abs(float(c[j, 0]) - a) <= 2.0 ** -23 * a and abs(float(c[j, 2]) - cc) <= 2.0 ** -23 * cc
    assert np.array_equal(c, R.table(R.learning_rates(lr, 2, Lc), T, friction, R.cycle_flags(Lc, 2, 0.25)))
    # the last quarter of the cycle (rows 15 .. 19), every second counted back from the last row
    assert [j for j in range(Lc) if c[j, 3]] == [15, 17, 19]
    assert [j for j in range(10) if sgmcmc.collect_flags(1, 10, 0.3)[j]] == [7, 8, 9]
    assert [j for j in range(4) if sgmcmc.collect_flags(3, 4, 0.1)[j]] == [3]                  # at least the cycle's last row


# ---------------------------------------------------------------------------------------------- the restatement itself
def test_restated_noise_is_the_oracle_generator_on_word_3():
    from oracle import bnn_oracle as O
    e = R.noise(SEED, 5, 7, 1201)
    assert e.shape == (1201,) and e.dtype == np.float32 and np.isfinite(e).all()
    # one element by hand: i = 1102 -> group 275, slot 2
    r = O.philox4x32(np.uint32(275), np.uint32(7), np.uint32(5), np.uint32(3), SEED & 0xFFFFFFFF, SEED >> 32)
    assert O.box_muller(r[2], r[3])[0] == e[1102] and O.box_muller(r[0], r[1])[1] == e[1101]
    # a prefix does not depend on numel; tensors, steps and the epsilon map's word 3 = 0 are other streams
    assert np.array_equal(R.noise(SEED, 5, 7, 37), e[:37])
    for other in (R.noise(SEED, 4, 7, 1201), R.noise(SEED, 5, 8, 1201), R.noise(SEED + 1, 5, 7, 1201),
                  O.philox_normal(SEED, 5, 7, 1, 1201)[0]):
        assert not np.array_equal(other, e) and abs(np.corrcoef(other, e)[0, 1]) < 0.15
    assert np.array_equal(R.noise(SEED, 0, 2 ** 32 - 1, 5), R.noise(SEED, 0, -1, 5))
    big = R.noise(SEED, 15, 0, 1 << 16)
    assert abs(big.mean()) < 4 / 256 and abs(big.var() - 1) < 0.03


def test_restated_fma_is_correctly_rounded():
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal(4000).astype(np.float32), rng.standard_normal(4000).astype(np.float32)
    c = (rng.standard_normal(4000) * 10.0 ** rng.integers(-8, 3, 4000)).astype(np.float32)
    # a b + c half way between two floats but for the product's 2^-46 tail: a separate multiply and add rounds it down
    a[0], b[0], c[0] = np.float32(1 + 2.0 ** -23), np.float32(1 + 2.0 ** -23), np.float32(2.0 ** -24 - 2.0 ** -22)
    got = R.fma32(a, b, c)

    def exact(x, y, z):
        f = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo = np.float32(float(f))                                  # (float(Fraction) rounds correctly to fp64; candidates from it)
        cands = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
        best = min(cands, key=lambda q: (abs(Fraction(float(q)) - f), int(np.float32(q).view(np.uint32)) & 1))
        return np.float32(best)
    want = np.array([exact(x, y, z) for x, y, z in zip(a, b, c)], dtype=np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    p, v = R.update(np.float32(0.3), np.float32(-0.2), np.float32(0.01), np.float32(1.5), 468.75, 0.5, 0.05, 0.9, 0.1)
    g = 468.75 * 0.01 + 0.5 * 0.3
    v64 = 0.1 * 1.5 + (-0.05 * g + 0.9 * -0.2)
    assert abs(float(v) - v64) < 1e-6 and abs(float(p) - (0.3 + v64)) < 1e-6


def test_restated_ring_layout_and_chain():
    assert R.layout([1, 37, 70 * 37, 1201]) == ([0, 64, 128, 128 + 2624], 128 + 2624 + 1216)
    assert R.layout([64, 65]) == ([0, 64], 192)
    from bnn_hip import ops
    assert ops.bank_layout([1, 37, 70 * 37, 1201]) == ((0, 64, 128, 2752), 3968)
    assert [R.ring_slot(c, 3) for c in range(7)] == [0, 1, 2, 0, 1, 2, 0] and R.ring_slot(2 ** 32 + 1, 2) == 1
    # the issue's ring: L = 5, flags [0, 0, 1, 0, 1], burn_in 3, capacity 2, 12 steps -> steps 4, 7, 9 collect
    tab = R.table([0.1, 0.2, 0.3, 0.4, 0.5], flags=[0, 0, 1, 0, 1])
    bank = np.full((2, 192), 7.0, dtype=np.float32)
    ch = R.Chain([np.ones(3, np.float32), np.ones(65, np.float32)], tab, grad_scale=1.0, tau=1.0, momentum=False, burn_in=3,
                 bank=bank, seed=SEED)
    after = {}
    for k in range(12):
        ch.step([np.zeros(3, np.float32), np.zeros(65, np.float32)])
        after[k] = [t.copy() for t in ch.p]
    assert ch.k == 12 and ch.collected == 3 and ch.rows_used == [0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 1]
    assert np.array_equal(bank[0, :3], after[9][0]) and np.array_equal(bank[0, 64:129], after[9][1])
    assert np.array_equal(bank[1, :3], after[7][0]) and not np.array_equal(after[4][0], after[9][0])
    assert (bank[:, 3:64] == 7.0).all() and (bank[:, 129:] == 7.0).all()                                       # the padding is never written


@pytest.mark.parametrize("name,lr,friction", [("sgld", 0.5, None), ("sghmc", 0.1, 0.3)])
def test_update_rule_samples_the_stationary_law(name, lr, friction):
    """16 384 independent elements, 200 steps from zero at grad = 0, tau = 1, T = 1: the variance within 5 %, the mean within 4
    standard errors and the lag-1 correlation within 0.01 of the linear chain's stationary law (about 4.5 standard errors of
    the estimators at this n; the transient rho(A)^200 is below 1e-15)."""
    n, tau = 16384, 1.0
    tab = R.table(R.learning_rates(lr, 1), 1.0, friction)
    ch = R.Chain([np.zeros(n, np.float32)], tab, grad_scale=1.0, tau=tau, momentum=friction is not None, seed=SEED)
    zero = [np.zeros(n, np.float32)]

    def run(k):
        ch.step(zero)
        return ch.p[0]
    var, mean, lag1 = R.chain_statistics(run, n, 200)
    ratio, got, want = R.check_statistics(var, mean, lag1, tab[0], tau, n)
    print(f"{name}: var / Sigma_pp = {ratio:.4f}, lag-1 = {got:.4f} against {want:.4f}, mean = {mean:.5f}")
    S, A = R.stationary(*[float(v) for v in tab[0, :3]], tau)
    if friction is None:                                          # p' = (1 - a) p + c eps in closed form
        a, c = float(tab[0, 0]), float(tab[0, 2])
        assert abs(S[0, 0] - c * c / (1 - (1 - a) ** 2)) < 1e-12 and abs((A @ S)[0, 0] / S[0, 0] - (1 - a)) < 1e-12
    assert np.abs(A @ S @ A.T + float(tab[0, 2]) ** 2 - S).max() < 1e-12
