"""The fp64 restatement of the LR layer forward (tests/lr_fwd_ref.py), its bound and its cells, proven without a GPU:
 1. the restatement equals the oracle (oracle/bnn_oracle.py: lr_linear, lr_linear_mean evaluated in float64) to 1e-12 relative
    in every regular cell, and its bf16 rounding points equal the layer step of network_forward_bf16 run in float64;
 2. the reference's own fp32 arithmetic (lr_linear on fp32 tensors) and an fp32 emulation of the kernels' operation order, in
    fp32 and in bf16 math, lie inside the bound in every regular cell and for every input kind: the bound is a condition on
    the INPUTS, not on one implementation;
 3. eight seeded wrong variants of the emulation -- each a plausible kernel slip -- exceed the bound in a regular cell, which
    the test names;
 4. conditions: nothing is excluded from a comparison, tie_share <= 1 % over the bf16 cells, the cell counts."""
import numpy as np
import pytest
import torch

import fwd_stats_ref as F
import lr_fwd_ref as R
from oracle import bnn_oracle as O

S, B, K, N = 4, 8, 16, 16
REL = 1e-12
REGULAR = tuple(c for c in R.cells() if c.tag == "regular")


def _inputs(cell, kind="a"):
    return (R.kind_x(kind, B, K),) + F.cell_params(cell, N, K, lr=True) + R.lr_eps(S, B, N)


def _cond(ref, x, p, ea):
    """What a relative 1e-12 is relative to: sum |x| |M| + sqrt(v) |eps| + |b|."""
    return np.abs(np.asarray(x, np.float64)) @ np.abs(p[0].astype(np.float64)) + np.sqrt(ref.v) * np.abs(ea) + np.abs(ref.bias)[:, None, :]


# ------------------------------------------------------------------------------------------ 1. restatement == the oracle
def test_restatement_equals_the_oracle_in_fp64():
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    worst = 0.0
    for c in REGULAR:
        x, *p, ea, eb = _inputs(c)
        ref = R.lr_ref(x, *p, ea, eb)
        cond = _cond(ref, x, p, ea)
        for s in range(S):
            y, _, _ = O.lr_linear(t(x), *(t(a) for a in p), t(ea[s]), t(eb[s]), 1.0, want_kl=False)
            e = np.abs(y.numpy() - ref.y[s])
            assert bool(np.all(e <= REL * cond[s])), (c.name, s)
            worst = max(worst, float((e / np.maximum(cond[s], 1e-300)).max()))
        mean = O.lr_linear_mean(t(x), t(p[0]), t(p[2])).numpy()
        assert bool(np.all(np.abs(mean - ref.y_mean[0]) <= REL * cond[0])), c.name
        zero = R.lr_ref(x, *p, None, None)                     # BNN_EPS_ZERO: the same numbers through the sampling formula
        assert np.array_equal(zero.y[0], ref.y_mean[0]) and np.all(zero.hfac == 0), c.name
    print(f"largest relative difference from the oracle in float64: {worst:.2e}")


def test_rounding_points_equal_the_oracles_bf16_layer_step_in_fp64(monkeypatch):
    """network_forward_bf16 over ONE layer is that layer's step followed by ReLU.  Its _bf16 returns float32; evaluated in
    float64 the helper has to keep the dtype (fp64 -> fl32 -> bf16, the kernels' order of roundings, is what it then does)."""
    monkeypatch.setattr(O, "_bf16", lambda v: v.to(torch.float32).to(torch.bfloat16).to(v.dtype))
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    worst = 0.0
    for c in REGULAR:
        x, *p, ea, eb = _inputs(c)
        ref = R.lr_ref(x, *p, ea, eb, math="bf16", relu=True)
        cond = _cond(ref, x, p, ea)
        net = O.NetParams([tuple(t(a) for a in p)], "regression", K, True, O.Prior(False, 1.0))
        for s in range(S):
            y = O.network_forward_bf16(net, t(x), [t(ea[s]), t(eb[s])])[0].numpy()
            e = np.abs(y - ref.y[s])
            assert bool(np.all(e <= REL * cond[s])), (c.name, s)
            worst = max(worst, float((e / np.maximum(cond[s], 1e-300)).max()))
    print(f"bf16 rounding points against network_forward_bf16 in float64: largest relative difference {worst:.2e}")


def test_split_bf16_mean_is_the_sum_of_the_three_plane_products():
    """bf16x3: the restated mean over the planes (x, x_lo) and (M_hi, M_lo) equals O.linear_bf16x3 up to the latter's fp32
    accumulation, and the fp32 product x . M to the 2^-16 the dropped lo . lo term and the lo planes' rounding leave."""
    c = REGULAR[3 * 8 + 4]
    x, *p, ea, eb = _inputs(c)
    xt = torch.from_numpy(x)
    hi = xt.to(torch.bfloat16)
    lo = (xt - hi.float()).to(torch.bfloat16)
    ref = R.lr_ref(hi, *p, ea, eb, math="bf16x3", x_lo=lo, x_sq=(xt * xt).to(torch.bfloat16))
    want = O.linear_bf16x3(xt, torch.from_numpy(p[0]).t(), torch.zeros(N)).numpy()
    am = np.abs(x.astype(np.float64)) @ np.abs(p[0].astype(np.float64))
    assert np.all(np.abs(want - ref.m[0]) <= (3 * K + 16) * R.U * am)
    assert np.all(np.abs(x.astype(np.float64) @ p[0].astype(np.float64) - ref.m[0]) <= 2.0 ** -15 * am)


# ---------------------------------------------------------------------- 2. the bound is a condition on the inputs
def _shares(got, ref):
    """Largest share of the bound of (y, v, hfac): EVERY element, none excluded."""
    return tuple(F.share(g, r, b) for g, r, b in zip(got, (ref.y, ref.v, ref.hfac), (ref.b_y, ref.b_v, ref.b_hfac)))


@pytest.mark.parametrize("kind", ["a", "b", "c"])
def test_reference_formula_and_emulation_lie_inside_the_bound(kind):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    worst, ties = {}, []
    for c in REGULAR:
        x, *p, ea, eb = _inputs(c, kind)
        for relu in (False, True):
            ref = R.lr_ref(x, *p, ea, eb, relu=relu)
            y = np.stack([O.lr_linear(t(x), *(t(a) for a in p), t(ea[s]), t(eb[s]), 1.0, want_kl=False)[0].numpy() for s in range(S)])
            sh = F.share(np.maximum(y, 0) if relu else y, ref.y, ref.b_y)
            assert sh <= 1.0, (c.name, kind, "reference fp32", sh)
            worst["reference fp32"] = max(worst.get("reference fp32", 0.0), sh)
            for math in ("f32", "bf16"):
                r = ref if math == "f32" else R.lr_ref(x, *p, ea, eb, math=math, relu=relu)
                sh = _shares(R.emu_lr(x, *p, ea, eb, math=math, relu=relu), r)
                assert max(sh) <= 1.0, (c.name, kind, math, relu, sh)
                worst[math] = tuple(max(a, b) for a, b in zip(worst.get(math, (0.0,) * 3), sh))
                if math == "bf16" and not relu:
                    ties.append(r.info["tie_share"])
        if kind == "b":                                        # the all-zero row: v = 0, hfac = 0, y = b with the bias's bound alone
            ref = R.lr_ref(x, *p, ea, eb)
            assert np.all(ref.v[:, 1] == 0) and np.all(ref.b_v[:, 1] == 0) and np.all(ref.hfac[:, 1] == 0) and np.all(ref.b_hfac[:, 1] == 0), c.name
            assert np.array_equal(ref.y[:, 1], ref.bias), c.name
        if kind == "c":                                        # x^2 underflows: hfac is unbounded, v and y stay bounded
            assert np.all(np.isinf(ref.b_hfac[1:])) and np.all(np.isfinite(ref.b_v)) and np.all(np.isfinite(ref.b_y)), c.name
    # (one tie among a cell's 256 weights is 0.4 % already: the share is held over the cells together, and cell by cell on the
    # device's larger shapes below)
    assert len(ties) == 97 and float(np.mean(ties)) <= 0.01, (max(ties), np.mean(ties))
    print(f"kind ({kind}): largest share of the bound  reference fp32 y {worst['reference fp32']:.3f}  "
          + "  ".join(f"emulation {m}: y {worst[m][0]:.3f} v {worst[m][1]:.3f} hfac {worst[m][2]:.3f}" for m in ("f32", "bf16"))
          + f"  | tie_share over the bf16 cells: mean {np.mean(ties):.4f} largest {max(ties):.4f}")


def test_tie_share_on_the_shapes_the_device_runs():
    """tie_share <= 1 % holds for the reference alone on every weight shape of tests/test_gpu_lr_fwd.py: over each shape's cells
    together, and cell by cell from 4096 weights on (below that a handful of ties decides the figure)."""
    worst = 0.0
    for (k, n) in ((16, 16), (40, 64), (104, 128), (24, 10), (100, 13), (104, 20), (1, 7), (8, 16), (8, 128), (104, 72), (264, 68), (40, 72),
                   (40, 136), (40, 520), (40, 10), (33, 21)):
        ties = total = 0
        for c in (R.cells() if (k, n) == (16, 16) else R.cells("rho")):
            if c.tag != "regular":
                continue
            rho = F.cell_params(c, n, k, lr=True)[1].astype(np.float64)
            s2 = F.softplus64(rho) ** 2
            _, slack = R.bf16_tie(s2, (2 * F.rel_sigma(rho) + R.U) * s2)
            ties, total = ties + int((slack > 0).sum()), total + rho.size
            assert rho.size < 4096 or float((slack > 0).mean()) <= 0.01, (c.name, k, n, float((slack > 0).mean()))
        assert ties <= 0.01 * total, (k, n, ties, total)
        worst = max(worst, ties / total)
    print(f"largest tie_share over the device shapes: {worst:.4f}")
    assert worst <= 0.01


# ------------------------------------------------------------------------------------------------- 3. the cells
def test_cell_counts_and_regimes():
    cs = R.cells()
    tags = [c.tag for c in cs]
    assert (tags.count("regular"), tags.count("band"), tags.count("edge")) == (97, 1, 2) and len({c.name for c in cs}) == 100
    red = R.cells("rho")
    assert [c.tag for c in red].count("regular") == 13 and len(red) == 16 and {c.rho for c in red} >= set(F.RHO_LEVELS)
    assert sorted({c.rho for c in cs if c.tag != "regular"}) == [-200.0, -100.0, 89.0]
    ea, eb = R.lr_eps(S, B, N)
    for s in range(S):
        assert np.abs(ea[s]).max() <= F.EPS_SCALES[s] and np.abs(eb[s]).max() <= F.EPS_SCALES[s]
        assert s == 0 or np.abs(ea[s]).max() > 0.9 * F.EPS_SCALES[s]
    assert np.abs(R.lr_eps(1, B, N, shift=2)[0]).max() > 2.7
    xb = R.kind_x("b", B, K)
    assert np.all(xb >= 0) and np.all(xb[1] == 0) and np.all(xb[:, 2] == 0) and 0.35 < float((xb == 0).mean()) < 0.75
    xc = R.kind_x("c", B, K).astype(np.float64)
    assert np.all(xc * xc < F.MIN_NORMAL) and np.all(xc == R.kind_x("a", B, K).astype(np.float64) * 2.0 ** -70)
    # the |mu| = 0 cells expose sqrt(v) by itself; the edges are what fp32 makes of them
    c0 = [c for c in cs if c.tag == "regular" and c.mu == 0][0]
    assert np.all(F.cell_params(c0, N, K, lr=True)[0] == 0)
    for c in cs:
        rho = F.cell_params(c, N, K, lr=True)[1]
        sg = torch.log1p(torch.exp(torch.from_numpy(rho)))
        if c.rho == 89.0:
            assert bool(torch.isinf(sg).all()), c.name
        elif c.rho == -200.0:
            assert bool((sg == 0).all()), c.name
        elif c.rho == F.RHO_BAND:
            assert bool(((sg > 0) & (sg < 2.0 ** -126)).all()) and bool((sg * sg == 0).all()), c.name
        else:
            assert bool(torch.isfinite(sg).all()) and bool((sg * sg > 2.0 ** -126).all()), c.name


# ------------------------------------------------------------------------------------------ 4. seeded wrong variants
def _largest_share(variant):
    math = "bf16" if variant == "x2_not_rerounded" else "f32"
    relu = variant == "relu_before_bias"
    worst, where = 0.0, None
    for c in REGULAR:
        x, *p, ea, eb = _inputs(c)
        ref = R.lr_ref(x, *p, ea, eb, math=math, relu=relu)
        sh = _shares(R.emu_lr(x, *p, ea, eb, math=math, relu=relu, variant=variant), ref)
        for name, v in zip(("y", "v", "hfac"), sh):
            if v > worst:
                worst, where = v, f"{c.name} ({name})"
    return worst, where


def _init_range_catches(variant):
    """Would the suite's init-range tolerances have caught it?  |mu| <= 0.2, rho in [-5, -4], x in [0, 1], N(0, 1) epsilon:
    y at rtol 2e-5 of its scale (fp32 math) or 2e-2 (bf16 math) -- v and hfac were compared with no reference at all."""
    rs = np.random.RandomState(7)
    k, n, b = 64, 32, 16
    p = (rs.uniform(-0.2, 0.2, (k, n)), rs.uniform(-5, -4, (k, n)), rs.uniform(-0.2, 0.2, n), rs.uniform(-5, -4, n))
    p = tuple(np.ascontiguousarray(a, np.float32) for a in p)
    x = rs.uniform(0, 1, (b, k)).astype(np.float32)
    ea, eb = rs.standard_normal((1, b, n)).astype(np.float32), rs.standard_normal((1, n)).astype(np.float32)
    math = "bf16" if variant == "x2_not_rerounded" else "f32"
    relu = variant == "relu_before_bias"
    ref = R.lr_ref(x, *p, ea, eb, math=math, relu=relu)
    y = R.emu_lr(x, *p, ea, eb, math=math, relu=relu, variant=variant)[0]
    return float(np.abs(y - ref.y).max()) > (2e-5 if math == "f32" else 2e-2) * float(np.abs(ref.y).max())


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_seeded_wrong_variants_break_the_bound(variant):
    """The last k element missing from the variance product; a clamped tail element counted twice; sigma^2 rounded to bf16 in fp32
    math; x^2 of the un-rounded x in bf16 math; sqrt(v) rounded to bf16; sigma_b eps_b dropped; ReLU ahead of the bias; hfac from
    sqrt(v + 1e-8): each exceeds the bound in a regular cell."""
    worst, where = _largest_share(variant)
    print(f"{variant}: largest share of the bound {worst:.3g} at {where}; the init-range tolerance on y "
          f"{'would have caught it' if _init_range_catches(variant) else 'does NOT catch it'}")
    assert worst > 1.0, (variant, worst, where)
