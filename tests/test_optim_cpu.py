"""The fp64 restatement of the fused optimiser steps (tests/optim_ref.py) and its bound, proven without a GPU:
 1. the restatement equals torch.optim.Adam / torch.optim.SGD in float64 over 5 steps, to 1e-12 relative: the same rule;
 2. the fp32 emulation of the kernels' arithmetic lies inside the bound at every case of the GPU matrix
    (tests/test_gpu_optim.py) and every output element, the largest share err / bound printed per case;
 3. every seeded wrong variant of that emulation breaks the bound, by more than 4 x, at the case named for it -- and the
    inputs hold the elements that make this possible;
 4. the geometry table puts every kind of chunk boundary into a launch's chunk table."""
import numpy as np
import pytest
import torch

import optim_ref as R


# ------------------------------------------------------------------------------------------ 1. restatement == torch
def _rel_equal(got, want, what):
    got, want = np.asarray(got), want.detach().numpy()
    err = np.abs(got - want)
    assert (err <= 1e-12 * np.abs(want)).all(), (what, float((err / np.maximum(np.abs(want), 1e-300)).max()))


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adam_restatement_equals_torch_adam_in_fp64(wd):
    rs = np.random.RandomState(11)
    ps = [torch.nn.Parameter(torch.from_numpy(rs.standard_normal(n))) for n in (7, 33, 100)]
    kw = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=wd)
    opt = torch.optim.Adam(ps, lr=kw["lr"], betas=(kw["b1"], kw["b2"]), eps=kw["eps"], weight_decay=wd)
    mine = [(p.detach().numpy().copy(), np.zeros(p.numel()), np.zeros(p.numel())) for p in ps]
    for step in range(1, 6):
        gs = [rs.standard_normal(p.numel()) * 10.0 ** rs.randint(-3, 2) for p in ps]
        for p, g in zip(ps, gs):
            p.grad = torch.from_numpy(g.copy())
        opt.step()
        mine = [R.adam_ref(p, g, m, v, step=step, want_bound=False, **kw)[0] for (p, m, v), g in zip(mine, gs)]
        for i, (p, (p1, m1, v1)) in enumerate(zip(ps, mine)):
            _rel_equal(p1, p, ("p", step, i))
            _rel_equal(m1, opt.state[p]["exp_avg"], ("m", step, i))
            _rel_equal(v1, opt.state[p]["exp_avg_sq"], ("v", step, i))


@pytest.mark.parametrize("wd", [0.0, 1e-3])
def test_sgd_restatement_equals_torch_sgd_in_fp64(wd):
    rs = np.random.RandomState(12)
    ps = [torch.nn.Parameter(torch.from_numpy(rs.standard_normal(n))) for n in (7, 33, 100)]
    opt = torch.optim.SGD(ps, lr=0.05, weight_decay=wd)
    mine = [p.detach().numpy().copy() for p in ps]
    for step in range(5):
        gs = [rs.standard_normal(p.numel()) for p in ps]
        for p, g in zip(ps, gs):
            p.grad = torch.from_numpy(g.copy())
        opt.step()
        mine = [R.sgd_ref(p, g, lr=0.05, wd=wd, want_bound=False)[0] for p, g in zip(mine, gs)]
        for i, (p, p1) in enumerate(zip(ps, mine)):
            _rel_equal(p1, p, (step, i))


# ------------------------------------------------------------------------------------------ 2. fp32 inside the bound
def _emul_shares(name, bf16=False, variant=None):
    c = R.ADAM_CASES[name]
    got = R.adam_emul_list(R.adam_inputs(name, bf16), R.scalars(c), variant)
    return R.adam_shares(got, R.adam_expected(name, bf16))


@pytest.mark.parametrize("name", list(R.ADAM_CASES))
def test_adam_emulation_lies_inside_the_bound(name):
    for bf16 in (False, True):
        sh = _emul_shares(name, bf16)
        print(f"{name:36s} {'bf16' if bf16 else 'fp32'} g  share of the bound: " + "  ".join(f"{k}' {s:.3f}" for k, s in sh.items()))
        assert max(sh.values()) < 1.0, (name, bf16, sh)


def _sgd_emul_share(name, variant=None):
    c = R.SGD_CASES[name]
    got = [R.sgd_emul(t["p"], t["g"], lr=c["lr"], wd=c["wd"], variant=variant) for t in R.sgd_inputs(name)]
    return R.sgd_share(got, R.sgd_expected(name))


@pytest.mark.parametrize("name", list(R.SGD_CASES))
def test_sgd_emulation_lies_inside_the_bound(name):
    sh = _sgd_emul_share(name)
    print(f"{name:24s} share of the bound: p' {sh:.3f}")
    assert sh < 1.0, (name, sh)


def test_share_counts_a_nan_and_an_error_over_a_zero_bound_as_infinite():
    ref, bound = np.array([1.0, 0.0]), np.array([1e-7, 0.0])
    assert R.share(np.array([1.0, 0.0]), ref, bound) == 0.0
    assert R.share(np.array([np.nan, 0.0]), ref, bound) == np.inf
    assert R.share(np.array([1.0, 1e-30]), ref, bound) == np.inf
    assert R.share(np.array([1.0, 0.0]), ref, np.array([np.nan, 0.0])) == 0.0      # (an exact result needs no bound)
    assert R.share(np.array([1.1, 0.0]), ref, np.array([np.nan, 0.0])) == np.inf


# ------------------------------------------------------------------------------------------ 3. wrong variants outside
# the case at which each variant must be caught: chosen by what exercises it, not by what the emulation gives
ADAM_VARIANT_CASE = {
    "no_eps":            "s7-wd0-eps0.001-b0.9_0.999",       # sqrt(v') around and below eps
    "eps_in_sqrt":       "s7-wd0-eps0.001-b0.9_0.999",
    "no_bc2":            "s2-wd0-eps1e-08-b0.9_0.999",       # sqrt(bc2) = 0.045
    "no_bc1":            "s2-wd0-eps1e-08-b0.9_0.999",       # bc1 = 0.19
    "step_plus_1":       "s1-wd0-eps1e-08-b0.9_0.999",
    "powf":              "s1000-wd0-eps1e-08-b0.9_0.999",    # 0.999f ^ 1000: 1000 x the cast error of 0.999
    "step_size_1.001":   "s1000000-wd0-eps1e-08-b0.9_0.999",
    "adamw":             "s7-wd0.01-eps1e-08-b0.9_0.999",
    "wd_ignored":        "s7-wd0.01-eps1e-08-b0.9_0.999",
    "last_unwritten":    "geo16",
    "group_from_chunk0": "geo16",
}
SGD_VARIANT_CASE = {"wd_ignored": "sgd-regime-wd0.001", "plus_lr": "sgd-regime-wd0", "lr_bf16": "sgd-geo16-wd0"}


def test_every_variant_has_its_case():
    assert set(ADAM_VARIANT_CASE) == set(R.ADAM_VARIANTS) and set(SGD_VARIANT_CASE) == set(R.SGD_VARIANTS)
    assert set(ADAM_VARIANT_CASE.values()) <= set(R.ADAM_CASES) and set(SGD_VARIANT_CASE.values()) <= set(R.SGD_CASES)


@pytest.mark.parametrize("variant", R.ADAM_VARIANTS)
def test_seeded_wrong_adam_breaks_the_bound(variant):
    name = ADAM_VARIANT_CASE[variant]
    sh = _emul_shares(name, variant=variant)
    print(f"{variant:18s} at {name}: " + "  ".join(f"{k}' {s:.3g}" for k, s in sh.items()))
    assert max(sh.values()) > 4.0, (variant, name, sh)


@pytest.mark.parametrize("variant", R.SGD_VARIANTS)
def test_seeded_wrong_sgd_breaks_the_bound(variant):
    name = SGD_VARIANT_CASE[variant]
    sh = _sgd_emul_share(name, variant)
    print(f"{variant:18s} at {name}: p' {sh:.3g}")
    assert sh > 4.0, (variant, name, sh)


def test_late_steps_hide_what_early_steps_show():
    """Why steps 1, 2 and 7 stay in the table: at step 10^6 both bias corrections are 1 and `no_bc2`, `step_plus_1` give
    the honest kernel's bits."""
    name = "s1000000-wd0-eps1e-08-b0.9_0.999"
    for variant in ("no_bc2", "no_bc1", "step_plus_1"):
        assert max(_emul_shares(name, variant=variant).values()) < 1.0


def test_inputs_carry_the_edges():
    for name, c in R.REGIMES.items():
        (t,) = R.adam_inputs(name)
        p, g, m, v = (t[k] for k in "pgmv")
        n = p.size
        assert n == R.REGIME_N and all(a.dtype == np.float32 and not a.flags.writeable for a in (p, g, m, v))
        nz = np.abs(g[g != 0])
        assert nz.min() >= 1e-10 * (1 - 1e-6) and nz.max() <= 1e2 * (1 + 1e-6) and nz.min() < 1e-9 and nz.max() > 10.0
        assert (v[v != 0] >= 1e-24).all() and (v >= 0).all()          # normal fp32, as m: no denormals
        assert (np.abs(m[m != 0]) >= 1e-24).all()
        assert (p == 0).sum() >= n // 32 and ((p != 0) & (np.abs(p) <= 1e-6)).sum() >= n // 32
        if c["eps"] > 0:                                            # 0 / eps
            z = (g == 0) & (m == 0) & (v == 0) & ((p == 0) | (c["wd"] == 0))
            assert z.sum() >= n // 32 and z[-3:].any()
        if c["step"] == 1:
            assert not m.any() and not v.any()
        else:
            if c["eps"] > 0 or c["b2"] > 0:
                assert ((g == 0) & (m != 0) & (v > 0)).sum() >= n // 32
            if c["b1"] > 0:                                         # m' cancels: exactly, with the true b1, up to its own rounding
                (ref, _) = R.adam_ref(p, g, m, v, **R.scalars(c))
                cancel = (m != 0) & (np.abs(ref[1]) <= 2.0 ** -50 * np.abs(m))
                assert cancel.sum() >= n // 32 and cancel[-3:].any()
        # the rule's own 0 / 0 is nowhere
        (ref, bound) = R.adam_ref(p, g, m, v, **R.scalars(c))
        assert all(np.isfinite(a).all() for a in ref + bound)
        if c["eps"] > 0:                                            # eps decides: sqrt(v') / sqrt(bc2) within a factor 10 of it
            Rr = np.sqrt(ref[2]) / np.sqrt(1.0 - c["b2"] ** c["step"])
            near = (Rr >= c["eps"] / 10) & (Rr <= c["eps"] * 10)
            assert near.mean() >= 0.05, (name, near.mean())
    for name in R.ADAM_CASES:                                       # bf16 gradients are bf16 values, the rest is the same
        for a, b in zip(R.adam_inputs(name), R.adam_inputs(name, True)):
            assert np.array_equal(b["g"], R.bf16r(a["g"])) and not (b["g"].view(np.uint32) & 0xFFFF).any()
            assert all(np.array_equal(a[k], b[k]) for k in "pmv")


# ------------------------------------------------------------------------------------------ 4. geometry
def test_chunk_table_restates_the_walk():
    for sizes in [R.GEO16] + R.launches(R.GEO19) + list(R.GRIDS.values()):
        blocks = R.chunk_table(sizes)
        seen = [np.zeros(n, dtype=int) for n in sizes]
        for t, base, cnt in blocks:
            assert base % R.CHUNK == 0 and 0 < cnt <= R.CHUNK
            seen[t][base:base + cnt] += 1
        assert all((s == 1).all() for s in seen)                    # every element in exactly one block
        assert [t for t, _, _ in blocks] == sorted(t for t, _, _ in blocks)
    for n, sizes in R.GRIDS.items():
        assert len(R.chunk_table(sizes)) == n
    assert [len(s) for s in R.launches(R.GEO19)] == [16, 3] and [len(s) for s in R.launches(R.GEO17)] == [16, 1]


def test_geometry_covers_every_boundary_kind():
    """Per position in the chunk table (a tensor's first chunk or a later one; the launch's first block, a middle one, the
    last) every body: the whole chunk, the general loop ending on a full group of four, the scalar tail."""
    blocks = R.chunk_table(R.GEO16)
    kinds = {(R.block_kind(s, b), b[1] == 0) for s in R.launches(R.GEO19) for b in R.chunk_table(s)}
    assert kinds == {(k, f) for k in ("whole", "full4", "ragged") for f in (True, False)}
    # tensors of fewer than 4 elements, of exactly 4, tensors ending 1 short of / on / 1 past a chunk, at 1, 2 and 3 chunks
    assert {1, 2, 3, 4} <= set(R.GEO16)
    for k in (1, 2):
        assert {k * R.CHUNK - 1, k * R.CHUNK, k * R.CHUNK + 1} <= set(R.GEO16)
    assert 3 * R.CHUNK + 1 in R.GEO16
    assert R.GEO16[0] == 1 and R.GEO16[-1] == 1                     # the table's first and last block hold one element
    # a whole chunk directly followed by another tensor's first chunk, and a one-element tail chunk after whole chunks
    assert any(R.block_kind(R.GEO16, a) == "whole" and b[1] == 0 for a, b in zip(blocks, blocks[1:]))
    assert any(R.block_kind(R.GEO16, a) == "whole" and b[2] == 1 and b[1] > 0 for a, b in zip(blocks, blocks[1:]))
    # the regime tensor: the whole-chunk body and the scalar tail
    assert [R.block_kind((R.REGIME_N,), b) for b in R.chunk_table((R.REGIME_N,))] == ["whole", "ragged"]
    # the second launch of the 19- and 17-tensor calls starts its own table
    assert R.chunk_table(R.launches(R.GEO19)[1])[0] == (0, 0, R.CHUNK)


def test_arena_views_are_aligned_and_guarded():
    arrs = [np.arange(n, dtype=np.float32) for n in (1, 5, 4096, 7)]
    for itemsize in (4, 2):
        src = [R.bf16r(a) for a in arrs] if itemsize == 2 else arrs
        image, spans = R.arena(src, itemsize)
        assert R.arena_guards_intact(image, spans)
        per = 4 // itemsize
        for (o, n), a in zip(spans, src):
            assert o * itemsize % 16 == 0
            assert (image[o - R.GUARD * per:o] == image[0]).all() and (image[o + n:o + n + R.GUARD * per] == image[0]).all()
            back = image[o:o + n].astype(np.uint32) << 16 if itemsize == 2 else image[o:o + n]
            assert np.array_equal(back.view(np.float32), a)
        for o, n in spans:                                          # one element past the end, one before the start
            for at in (o + n, o - 1):
                hit = image.copy()
                hit[at] = 0
                assert not R.arena_guards_intact(hit, spans)
