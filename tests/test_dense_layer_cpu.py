"""The fp64 restatement of the dense layer (tests/dense_layer_ref.py) and its bound, proven without a GPU:
 1. the restatement equals torch autograd in fp64 on every case of the table: the forward formed with F.linear, relu and
    the restated masks; its backward gives g_w, g_b and g_x;
 2. the bound is honest: three fp32 evaluations -- torch's matmul, a sequential k-order loop and the kernels' staged walk --
    lie inside it at every element of every case, the largest share err / bound printed per case;
 3. the bound has power: every seeded wrong variant breaks it at every case it applies to;
 4. a bf16 output's two admissible neighbours differ on fewer than 1 % of a case's elements;
 5. the table reaches every class of every dimension and every variant of the launch."""
import pytest
import torch
import torch.nn.functional as F

import dense_layer_ref as R

F64 = torch.float64
FWD = list(R.FWD_CASES)
BWD = list(R.BWD_CASES)
AG_TOL = 1e-6            # of the bound: fp64 summation-order noise is 2^-29 of the fp32 bound and less


def _inside(got, want, bound, what):
    err = (got - want).abs()
    assert bool((err <= AG_TOL * bound).all()), (what, float((err / bound.clamp_min(1e-300)).max()))


# ------------------------------------------------------------------------------------------ 1. restatement == autograd
@pytest.mark.parametrize("name", FWD)
def test_forward_restatement_equals_autograd_forward_in_fp64(name):
    c, d, ref = R.FWD_CASES[name], R.fwd_inputs(name), R.fwd_reference(name)
    x, w = d["x"].to(F64), d["w"].to(F64)
    if c["math"] == "bf16":
        x, w = R.bf16r(x), R.bf16r(w)
    z = F.linear(x, w, None if d["b"] is None else d["b"].to(F64))
    if c["relu"]:
        z = torch.relu(z)
    y = z * R.masks(c["S"], c["B"], c["N"], c["p"], R.fwd_sample0(c))
    assert y.shape == ref.y.shape == (c["S"], c["B"], c["N"])
    assert torch.equal(y == 0, ref.y == 0)
    _inside(ref.y, y, ref.bound, name)
    if c["p"] > 0:
        kept = float((R.masks(c["S"], c["B"], c["N"], c["p"], R.fwd_sample0(c)) > 0).double().mean())
        assert 0.0 < kept < 1.0 or c["S"] * c["B"] * c["N"] < 8


@pytest.mark.parametrize("name", BWD)
def test_backward_restatement_equals_autograd_in_fp64(name):
    """h = y_scale relu(u) with u = x W^T + b shifted onto the case's saved output y (u + (y - u) is y's sign exactly, and
    +0 at both zeros, where relu's gradient is 0 like the kernel's y > 0); x = gx_scale relu(v) in gradient, the case's x in
    value.  d sum(h gy) / d (W, b, v) are g_w, g_b and g_x.  bf16 math: g_x from the rounded W and the rounded gradient of u."""
    c, d, ref = R.BWD_CASES[name], R.bwd_inputs(name), R.bwd_reference(name)
    B, K, N = c["B"], c["K"], c["N"]
    x0, gy, w0 = d["x"].to(F64), d["gy"].to(F64), d["w"].to(F64)
    v = x0.clone().requires_grad_(True)

    def make_x():
        if not c["mask"]:
            return v + 0
        r = torch.relu(v) * c["gx_scale"]
        return x0 + (r - r.detach())

    assert torch.equal(make_x().detach(), x0)
    w = w0.clone().requires_grad_(True)
    b = torch.zeros(N, dtype=F64, requires_grad=True)

    def head(lin):
        if not c["y"]:
            return (lin * gy).sum()
        y = d["y"].to(F64)
        u = lin + (y - lin).detach()
        assert torch.equal(u.detach() > 0, y > 0) and not bool((u.detach()[y == 0] != 0).any())
        return (torch.relu(u) * c["y_scale"] * gy).sum()

    g_w, g_b, g_x = torch.autograd.grad(head(F.linear(make_x(), w, b)), [w, b, v])
    if c["math"] == "bf16":
        lin = F.linear(make_x(), w, b)
        gz = torch.autograd.grad(head(lin), lin)[0]
        lin_r = F.linear(make_x(), R.bf16r(w0))
        g_x = torch.autograd.grad(lin_r, v, grad_outputs=R.bf16r(gz))[0]
    want = (g_w, g_b if c["gb"] else None, g_x if c["gx"] else None)
    for n, got, wnt, bnd in zip(R.BWD_NAMES, ref.grads, want, ref.bounds):
        assert (got is None) == (wnt is None), (name, n)
        if got is not None:
            _inside(got, wnt, bnd, (name, n))


# ------------------------------------------------------------------------------------------ 2. fp32 inside the bound
def _orders(c):
    width = R.STAGE if c["math"] == "bf16" else 4
    return (("matmul", R.mm_exact), ("sequential", R.mm_seq), ("staged", R.mm_staged(width)))


@pytest.mark.parametrize("name", FWD)
def test_forward_fp32_evaluations_lie_inside_the_bound(name):
    c, ref = R.FWD_CASES[name], R.fwd_reference(name)
    line = []
    for what, mm in _orders(c):
        got = R.fwd_run(name, dtype=torch.float32, mm=mm, want_bound=False).y
        sh = R.fwd_share(got, ref)
        line.append(f"{what} {sh:.3f}")
        assert sh <= 1.0, (name, what, sh)
    print(f"{name:24s} fp32 share of the bound: " + "  ".join(line) + f"  ties {ref.info['tie_share']:.4f}")
    assert bool(torch.isfinite(ref.bound).all())


@pytest.mark.parametrize("name", BWD)
def test_backward_fp32_evaluations_lie_inside_the_bound(name):
    c, ref = R.BWD_CASES[name], R.bwd_reference(name)
    for what, mm in _orders(c):
        got = R.bwd_run(name, dtype=torch.float32, mm=mm, want_bound=False).grads
        sh = R.bwd_shares(got, ref)
        print(f"{name:18s} {what:10s} fp32 share of the bound: "
              + "  ".join(f"{n} {s:.3f}" for n, s in zip(R.BWD_NAMES, sh) if s is not None))
        assert max(s for s in sh if s is not None) <= 1.0, (name, what, sh)
    for b in ref.bounds:
        assert b is None or bool(torch.isfinite(b).all())


# ------------------------------------------------------------------------------------------ 3. wrong variants break it
@pytest.mark.parametrize("name", FWD)
def test_forward_wrong_variants_break_the_bound(name):
    """The last k element dropped; the k tail zero-filled from a multiple of 8; row 64 read from row 63; the bias missing on
    the last column group; the mask group shifted by one column group, and by one sample; bf16 by truncation; the last
    sample run skipped."""
    c, ref = R.FWD_CASES[name], R.fwd_reference(name)
    line = []
    for variant in R.FWD_VARIANTS:
        if not R.fwd_applies(c, variant):
            continue
        worst = R.fwd_share(R.fwd_run(name, variant=variant, want_bound=False).y, ref)
        line.append(f"{variant} {worst:.2g}")
        assert worst > 1.0, (name, variant, worst)
    print(f"{name:24s} variants miss the bound by: " + "  ".join(line))


@pytest.mark.parametrize("name", BWD)
def test_backward_wrong_variants_break_the_bound(name):
    """The last k element of either reduction dropped; either k tail zero-filled from a multiple of 8; row 64 read from row
    63; the bias gradient missing on the last column group; y >= 0 for y > 0; y_scale or gx_scale omitted; bf16 by
    truncation; g_x from the unrounded gz in bf16 math."""
    c, ref = R.BWD_CASES[name], R.bwd_reference(name)
    line = []
    for variant in R.BWD_VARIANTS:
        if not R.bwd_applies(c, variant):
            continue
        sh = R.bwd_shares(R.bwd_run(name, variant=variant, want_bound=False).grads, ref)
        worst = max(s for s in sh if s is not None)
        line.append(f"{variant} {worst:.2g}")
        assert worst > 1.0, (name, variant, worst)
    print(f"{name:18s} variants miss the bound by: " + "  ".join(line))


def test_every_variant_applies_somewhere():
    for variant in R.FWD_VARIANTS:
        assert sum(R.fwd_applies(c, variant) for c in R.FWD_CASES.values()) >= 3, variant
    for variant in R.BWD_VARIANTS:
        assert sum(R.bwd_applies(c, variant) for c in R.BWD_CASES.values()) >= 3, variant


# ------------------------------------------------------------------------------------------ 4. the tie share
@pytest.mark.parametrize("name", [n for n in FWD if R.FWD_CASES[n]["y16"]])
def test_bf16_output_tie_share_is_below_one_percent(name):
    share = R.fwd_reference(name).info["tie_share"]
    print(f"{name:24s} ties {share:.4f}")
    assert share < 0.01


# ------------------------------------------------------------------------------------------ 5. the table
def test_the_table_reaches_every_class():
    fc, bc = R.FWD_CASES.values(), R.BWD_CASES.values()
    assert {1, 63, 64, 65, 130} <= {R.fwd_rows(c) for c in fc}
    assert {1, 3, 4, 63, 64, 65, 130} <= {c["N"] for c in fc}
    ks = {1, 7, 8, 12, 31, 32, 33, 40, 65, 100}
    assert ks <= {c["K"] for c in fc}
    assert ks <= {c["N"] for c in bc if c["gx"]} and ks <= {c["B"] for c in bc}
    assert {1, 5, 33, 65, 77, 130} <= {c["B"] for c in bc}
    assert {1, 3, 4, 63, 64, 65, 130} <= {c["K"] for c in bc} and {1, 3, 4, 63, 64, 65, 130} <= {c["N"] for c in bc}
    assert {1, 5, 10} <= {c["S"] for c in fc if c["shared"]} and 3 in {c["S"] for c in fc if not c["shared"]}
    assert R.plan_runs(64, 4, 10, True) == (3, 4)                  # runs of 4, 4 and 2
    for key, want in (("relu", {True, False}), ("bias", {True, False}), ("p", {0.0, 0.5, 0.9}), ("off", {0, 17, R.WRAP}),
                      ("counter", {None, 5}), ("math", {"f32", "bf16"})):
        assert {c[key] for c in fc} == want, key
    assert {(c["x16"], c["y16"]) for c in fc if c["math"] == "bf16"} == {(False, False), (False, True), (True, False), (True, True)}
    assert any(c["inc"] and c["p"] == 0 for c in fc)
    assert any(c["x16"] and c["K"] % 8 == 4 for c in fc)           # W takes vector loads, x scalar loads
    assert any(R.fwd_sample0(c) + c["S"] > 2 ** 32 for c in fc)    # the global sample index wraps inside a launch
    for key in ("y", "mask", "gb", "gx"):
        assert {c[key] for c in bc} == {True, False}, key
    assert {c["math"] for c in bc} == {"f32", "bf16"}
    assert 20 <= len(R.FWD_CASES) <= 30 and 20 <= len(R.BWD_CASES) <= 30
    c = R.FWD_CASES[R.BIG]
    assert -(-R.fwd_rows(c) // 128) * -(-c["N"] // 128) == 576 >= R.MIN_BLOCKS and c["math"] == "bf16" and c["p"] == 0
