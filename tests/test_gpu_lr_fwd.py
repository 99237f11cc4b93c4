"""The local-reparameterisation layer FORWARD of csrc/lr_linear.hip -- y (fp32 and bf16), the saved variance v, the backward
factor hfac, the bf16 copy y16 and the squares y_sq, the eval mean path -- on an MI355X against the fp64 restatement
tests/lr_fwd_ref.py, regime cell by regime cell and kernel form by kernel form (that module's docstring: what is restated, the
rounding points per math mode, the bound and its derivation; tests/test_lr_fwd_cpu.py proves the restatement against the
oracle, the bound wide enough for the reference's own fp32 arithmetic and tight enough for eight seeded slips).
One launch per cell and case, every weight of it in one (rho, |mu|) regime of fwd_stats_ref.lr_cells("lr-1"):
  regular cells    EVERY element of every output within its bound; y16 and y_sq bitwise the functions of the launch's own y;
  rho = 89         sigma = +inf: v non-finite everywhere, y and hfac non-finite or 0 (sign and NaN-ness free: 0 * inf);
  rho = -200, -100 sigma = 0 (the band's denormal sigma has sigma^2 = 0 in fp32 whether or not it is flushed): v = 0 and
                   hfac = 0 exactly, y within the eval path's bound of m + b_mu.
Every case asserts through ops.lr_plan that the geometry it means to exercise is the one launched (form, k_classes,
batch_rows, waves, k_slices) and test_the_case_table_covers_every_form that no row of the table below is empty; the K3r cases
(no plan: bnn_lr_final_fwd decides) assert that the layer's KL workspace came back untouched, which only the one-launch form
leaves so.  The smallest shape of each family runs the full 100-cell grid, the others the rho levels at |mu| = 0.05.

Measured on the MI355X: the raw v_sqrt_f32 of y's epilogue 1.3331 u (E_SQRT = 4; test_sqrt_error_constant re-measures it).
Input kind (c), x scaled by 2^-70 (x^2 below 2^-126): nothing is flushed in fp32 math -- the squares stay denormals and v comes
back non-zero from rho = -2 up, 0 below (the products vanish) --; in bf16 math bf16(x^2) is 0 (bf16 ends at 2^-133) and v = 0,
hfac = 0 in every cell.  y stays within its bound, which carries sqrt(dv) there.  The band rho = -100: v = 0, hfac = 0, y within
the bound of m + b_mu in every form.
The first run found K3a in bf16 math on an fp32 x squaring the UN-rounded x: v off by up to 2^-8 per term, 180 to 4900 times its
bound at rho = -20 in every such case (k3a-r4-bf16 y 530), invisible to the init-range tolerances (test_lr_fwd_cpu.py's variant
x2_not_rerounded); lr_fwd_body now squares the rounded fragment like every other form.
Largest share of the bound over the regular cells, afterwards (a bf16 y sits at up to 0.99 of its bound: half a bf16 ulp is
most of it; v and hfac at 0.85 - 0.98 in bf16 math on the larger shapes are elements whose sigma^2 lies at a rounding tie and
went to the other neighbour than fp64's -- lr_fwd_ref's tie term, one bf16 ulp of that operand, is nearly all of their bound):
                        y      v      hfac                                y      v      hfac
  k3a-r4-f32            0.338  0.235  0.228      k3a-kind-b-f32           0.270  0.315  0.324
  k3a-r4-f32-relu       0.982  0.225  0.228      k3a-kind-b-bf16          0.270  0.045  0.103
  k3a-r4-f32-x16        0.105  0.229  0.239      k3a-kind-c-f32           0.270  0.000  0.000
  k3a-r4-bf16           0.351  0.043  0.119      k3a-kind-c-bf16          0.270  0.000  0.000
  k3a-r4-bf16-x16       0.351  0.043  0.119      k3b-kind-b               0.988
  k3a-r2-f32            0.108  0.148  0.163      k3b-kind-c               0.275
  k3a-r2-bf16-x16       0.991  0.037  0.079      k3s-s1                   0.970  0.981  0.980
  k3a-r1-f32-x16        0.092  0.091  0.101      k3s-s1-xf32              0.899  0.954  0.951
  k3a-r1-bf16           0.950  0.977  0.976      k3s-shared               0.708  0.852  0.850
  k3a-mt2-f32           0.086  0.185  0.182      k3s-shared-spread        0.991  0.852  0.850
  k3a-mt2-bf16          0.077  0.042  0.092      k3s-per-sample           0.675  0.851  0.848
  k3a-philox            0.156  0.225  0.448      k3b-raw                  0.988
  k3a-edge-k100-n13     0.081  0.085  0.092      k3b-raw-y16              0.983
  k3a-edge-k100-bf16    0.048  0.023  0.038      k3b-prep-w4              0.976
  k3a-edge-b130         0.072  0.086  0.099      k3b-prep-w8              0.995
  k3a-edge-b130-bf16    0.082  0.944  0.941      k3b-prep-w16             0.989
  k3a-edge-k1           0.132  0.374  0.368      k3b-x3                   0.985
  k3a-edge-k1-bf16      0.131  0.000  0.144      k3b-x3-planes            0.985  (y + y_lo 0.953)
  k3a-edge-k8           0.108  0.307  0.291      k3r-parked               0.347  0.045
  k3a-edge-idle-wave    0.154  0.401  0.376      k3r-prepared-rt2         0.307  0.046
  eval-eps-zero         0.057  0.179  0.000      eval-eps-zero-bf16       0.011  0.053  0.000
  module sample=False   0.057 (f32)  0.013 (bf16)
"""
import collections

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fwd_stats_ref as F
import lr_fwd_ref as R
from bnn_hip import _lib as L
from bnn_hip import ops
from test_gpu_fwd_stats import Tally

SEED, LAYER_ID, OFFSET = 0x5EEDF00D12345678, 1, 3
BF = torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _stop_on_a_device_error():
    """An assertion that fails lets the next test run; an error of the device ends the session."""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as exc:                                   # noqa: BLE001
        pytest.exit(f"device error: {exc}", returncode=3)


def _up(a, dev):
    return None if a is None else (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(dev)


# ------------------------------------------------------------------------------------------------------- the case table
# row: what the table of forms calls it; shape (S, B, K, N); plan: what ops.lr_plan must say; grid: "full" | "rho"
def _c(row, shape, plan, *, math="f32", xdt="f32", ydt="f32", grid="rho", relu=False, eps="memory", x3d=False, kind="a", form=None,
       prepared=False, scratch=False, **kw):
    return dict(row=row, shape=shape, plan=plan, math=math, xdt=xdt, ydt=ydt, grid=grid, relu=relu, eps=eps, x3d=x3d, kind=kind,
                form=form, prepared=prepared, scratch=scratch, **kw)


def _tile(R_, MT, waves):
    return dict(form=L.FORM_TILE, k_classes=R_, batch_rows=16 * MT, waves=waves, k_slices=1)


def _gemm(waves):
    return dict(form=L.FORM_GEMM, k_classes=1, batch_rows=128, waves=waves, k_slices=1)


def _ksl(slices):
    return dict(form=L.FORM_GEMM_KSLICE, k_classes=1, batch_rows=128, waves=8, k_slices=slices)


T, G, KS = L.FORM_TILE, L.FORM_GEMM, L.FORM_GEMM_KSLICE
CASES = collections.OrderedDict([
    # ---- K3a tile: R = 4, 2, 1; MT = 8 and 2; fp32 and bf16 math, fp32 and bf16 x, fp32 and bf16 y
    ("k3a-r4-f32",          _c("k3a", (3, 8, 16, 16), _tile(4, 8, 1), grid="full", form=T)),
    ("k3a-r4-f32-relu",     _c("k3a", (3, 8, 16, 16), _tile(4, 8, 1), relu=True, ydt="bf16", form=T)),
    ("k3a-r4-f32-x16",      _c("k3a", (3, 8, 16, 16), _tile(4, 8, 1), xdt="bf16", form=T)),
    ("k3a-r4-bf16",         _c("k3a", (3, 8, 16, 16), _tile(4, 8, 1), math="bf16", grid="full", form=T)),
    ("k3a-r4-bf16-x16",     _c("k3a", (3, 8, 16, 16), _tile(4, 8, 1), math="bf16", xdt="bf16", grid="full", relu=True, form=T)),
    ("k3a-r2-f32",          _c("k3a", (15, 8, 40, 64), _tile(2, 8, 1), form=T)),
    ("k3a-r2-bf16-x16",     _c("k3a", (15, 8, 40, 64), _tile(2, 8, 1), math="bf16", xdt="bf16", ydt="bf16", form=T)),
    ("k3a-r1-f32-x16",      _c("k3a", (15, 8, 104, 128), _tile(1, 8, 4), xdt="bf16", relu=True, form=T)),
    ("k3a-r1-bf16",         _c("k3a", (15, 8, 104, 128), _tile(1, 8, 4), math="bf16", form=T)),
    ("k3a-mt2-f32",         _c("k3a", (1, 40, 24, 10), _tile(4, 2, 1), shift=2, form=T)),
    ("k3a-mt2-bf16",        _c("k3a", (1, 40, 24, 10), _tile(4, 2, 1), math="bf16", shift=3, relu=True, form=T)),
    ("k3a-philox",          _c("k3a", (3, 8, 16, 16), _tile(4, 8, 1), eps="philox", form=T)),
    # ---- K3a tile edges: K % 8 != 0 (guarded loads), N % 4 != 0 and N % F != 0, ragged B, two batch blocks, a K tail inside a
    # k-step with clamped 16-byte loads, K = 1, K smaller than one step, a wave that owns no k-step
    ("k3a-edge-k100-n13",   _c("k3a-edge", (3, 33, 100, 13), _tile(4, 2, 1), form=T)),
    ("k3a-edge-k100-bf16",  _c("k3a-edge", (3, 33, 100, 13), _tile(4, 2, 1), math="bf16", x3d=True, relu=True, form=T)),
    ("k3a-edge-b130",       _c("k3a-edge", (2, 130, 104, 20), _tile(4, 2, 1), shift=1, form=T)),
    ("k3a-edge-b130-bf16",  _c("k3a-edge", (2, 130, 104, 20), _tile(4, 2, 1), math="bf16", xdt="bf16", shift=2, form=T)),
    ("k3a-edge-k1",         _c("k3a-edge", (4, 5, 1, 7), _tile(4, 8, 1), form=T)),
    ("k3a-edge-k1-bf16",    _c("k3a-edge", (4, 5, 1, 7), _tile(4, 8, 1), math="bf16", form=T)),
    ("k3a-edge-k8",         _c("k3a-edge", (2, 8, 8, 16), _tile(4, 8, 1), shift=1, form=T)),
    ("k3a-edge-idle-wave",  _c("k3a-edge", (15, 40, 8, 128), _tile(1, 8, 2), form=T)),
    # ---- the input kinds (b) ReLU-like with a zero row and a zero column, (c) scaled by 2^-70
    ("k3a-kind-b-f32",      _c("kinds", (4, 8, 16, 16), _tile(4, 8, 1), kind="b", form=T)),
    ("k3a-kind-b-bf16",     _c("kinds", (4, 8, 16, 16), _tile(4, 8, 1), kind="b", math="bf16", form=T)),
    ("k3a-kind-c-f32",      _c("kinds", (4, 8, 16, 16), _tile(4, 8, 1), kind="c", form=T)),
    ("k3a-kind-c-bf16",     _c("kinds", (4, 8, 16, 16), _tile(4, 8, 1), kind="c", math="bf16", form=T)),
    ("k3b-kind-b",          _c("kinds", (2, 20, 40, 72), _gemm(4), kind="b", math="bf16", xdt="bf16", shift=1, form=G)),
    ("k3b-kind-c",          _c("kinds", (2, 20, 40, 72), _gemm(4), kind="c", math="bf16", xdt="bf16", shift=1, form=G)),
    # ---- K3s K-sliced: per-sample x; one x shared by S samples (es = S), from four samples on spread over the slice blocks; a
    # slice count that does not divide the k-steps (9 steps in 5 slices); N % 32 != 0
    ("k3s-s1",              _c("k3s", (1, 20, 104, 72), _ksl(4), math="bf16", xdt="bf16", grid="full", shift=2, form=KS, scratch=True)),
    ("k3s-s1-xf32",         _c("k3s", (1, 20, 104, 72), _ksl(4), math="bf16", shift=3, relu=True, form=KS, scratch=True)),
    ("k3s-shared",          _c("k3s-shared", (3, 33, 264, 68), _ksl(5), math="bf16", xdt="bf16", form=KS, scratch=True)),
    ("k3s-shared-spread",   _c("k3s-shared", (5, 33, 264, 68), _ksl(5), math="bf16", ydt="bf16", form=KS, scratch=True)),
    ("k3s-per-sample",      _c("k3s", (2, 33, 264, 68), _ksl(5), math="bf16", xdt="bf16", x3d=True, shift=1, form=KS, scratch=True)),
    # ---- K3b block GEMM on bf16 x + x_sq: 4 waves without w_frag; 4, 8 and 16 waves over lr_prepare fragments
    ("k3b-raw",             _c("k3b", (2, 20, 40, 72), _gemm(4), math="bf16", xdt="bf16", grid="full", shift=1, form=G)),
    ("k3b-raw-y16",         _c("k3b", (2, 20, 40, 72), _gemm(4), math="bf16", xdt="bf16", ydt="bf16", shift=2, relu=True, form=G)),
    ("k3b-prep-w4",         _c("k3b-prepared", (2, 20, 40, 136), _gemm(4), math="bf16", xdt="bf16", shift=1, form=G, prepared=True)),
    ("k3b-prep-w8",         _c("k3b-prepared", (86, 16, 40, 136), _gemm(8), math="bf16", xdt="bf16", ydt="bf16", form=G, prepared=True)),
    ("k3b-prep-w16",        _c("k3b-prepared", (52, 16, 40, 520), _gemm(16), math="bf16", xdt="bf16", relu=True, form=G, prepared=True)),
    # ---- K3b in split-bf16 math: lr_prepare(x3=True), x_lo; fp32 y, and the hi and lo y planes
    ("k3b-x3",              _c("k3b-x3", (2, 20, 40, 72), _gemm(4), math="bf16x3", xdt="bf16", grid="full", shift=1, form=G, prepared=True)),
    ("k3b-x3-planes",       _c("k3b-x3", (2, 20, 40, 72), _gemm(4), math="bf16x3", xdt="bf16", ydt="bf16", shift=2, relu=True, form=G, prepared=True)),
    # ---- K3r: lr_final_fwd's one-launch form (Philox eps): block-parked operands; prepared fragments with rt > 1
    ("k3r-parked",          _c("k3r", (2, 20, 40, 10), None, math="bf16", xdt="bf16", eps="philox", grid="full", final=True)),
    ("k3r-prepared-rt2",    _c("k3r", (64, 128, 40, 10), None, math="bf16", xdt="bf16", eps="philox", x3d=True, final=True, prepared=True)),
    # ---- the eval mean path
    ("eval-eps-zero",       _c("eval", (1, 9, 33, 21), _tile(4, 8, 1), eps="zero", grid="full", form=T)),
    ("eval-eps-zero-bf16",  _c("eval", (1, 9, 33, 21), _tile(4, 8, 1), eps="zero", math="bf16", relu=True, form=T)),
])
ROWS = ("k3a", "k3a-edge", "kinds", "k3s", "k3s-shared", "k3b", "k3b-prepared", "k3b-x3", "k3r", "eval")


def test_the_case_table_covers_every_form():
    """Every row of the table of forms is there, in the geometry named: a change to the dispatch fails the case's plan assertion,
    a change to this table fails here."""
    by_row = collections.defaultdict(list)
    for name, e in CASES.items():
        by_row[e["row"]].append(e)
    assert set(by_row) == set(ROWS)
    k3a = by_row["k3a"]
    assert {e["plan"]["k_classes"] for e in k3a} == {1, 2, 4} and {e["plan"]["batch_rows"] for e in k3a} == {128, 32}
    assert {(e["math"], e["xdt"]) for e in k3a} == {("f32", "f32"), ("f32", "bf16"), ("bf16", "f32"), ("bf16", "bf16")}
    assert {e["ydt"] for e in k3a} == {"f32", "bf16"} and {e["eps"] for e in k3a} == {"memory", "philox"}
    edge = {e["shape"] for e in by_row["k3a-edge"]}
    assert any(K % 8 for _, _, K, _ in edge) and any(K == 1 for _, _, K, _ in edge) and any(1 < K < 32 for _, _, K, _ in edge)
    assert any(K % 32 and K % 8 == 0 and K > 32 for _, _, K, _ in edge) and any(N % 4 for _, _, _, N in edge) and any(B > 128 for _, B, _, _ in edge)
    assert any(e["plan"]["waves"] > (e["shape"][2] + 31) // 32 for e in by_row["k3a-edge"])             # a wave without a k-step
    assert {e["kind"] for e in by_row["kinds"]} == {"b", "c"} and {e["math"] for e in by_row["kinds"]} == {"f32", "bf16"}
    assert all(e["plan"]["form"] == KS for e in by_row["k3s"] + by_row["k3s-shared"])
    assert {e["x3d"] for e in by_row["k3s"]} == {False, True} and {e["xdt"] for e in by_row["k3s"]} == {"f32", "bf16"}
    assert {e["shape"][0] >= 4 for e in by_row["k3s-shared"]} == {False, True} and all(not e["x3d"] and e["shape"][0] > 1 for e in by_row["k3s-shared"])
    assert any(((e["shape"][2] + 31) // 32) % e["plan"]["k_slices"] for e in by_row["k3s"] + by_row["k3s-shared"])
    assert any(e["shape"][3] % 32 for e in by_row["k3s"])
    assert all(e["plan"] == _gemm(4) and not e["prepared"] for e in by_row["k3b"]) and {e["ydt"] for e in by_row["k3b"]} == {"f32", "bf16"}
    assert {e["plan"]["waves"] for e in by_row["k3b-prepared"]} == {4, 8, 16} and all(e["prepared"] for e in by_row["k3b-prepared"])
    assert {e["ydt"] for e in by_row["k3b-prepared"]} == {"f32", "bf16"}
    assert all(e["math"] == "bf16x3" and e["prepared"] for e in by_row["k3b-x3"]) and {e["ydt"] for e in by_row["k3b-x3"]} == {"f32", "bf16"}
    assert {e["prepared"] for e in by_row["k3r"]} == {False, True} and all(e["eps"] == "philox" and e.get("final") for e in by_row["k3r"])
    assert any(_k3r_tiles(e) > 1 for e in by_row["k3r"]) and any(_k3r_tiles(e) == 1 for e in by_row["k3r"])
    assert all(e["eps"] == "zero" for e in by_row["eval"])
    assert {n for n, e in CASES.items() if e["grid"] == "full"} == {"k3a-r4-f32", "k3a-r4-bf16", "k3a-r4-bf16-x16", "k3s-s1", "k3b-raw", "k3b-x3",
                                                                    "k3r-parked", "eval-eps-zero"}


def _k3r_tiles(e):
    """LrRows.rt as bnn_lr_final_fwd sets it: two 16-row tiles per block over prepared fragments once S (RB + 1) > 512."""
    S, B, _, _ = e["shape"]
    rb = (B + 15) // 16
    return min(rb, 2) if e["prepared"] and S * (rb + 1) > 512 else 1


# ------------------------------------------------------------------------------------------------------------ one launch
MATH = {"f32": L.MATH_F32, "bf16": L.MATH_BF16, "bf16x3": L.MATH_BF16X3}
Launch = collections.namedtuple("Launch", "out ref")


def _inputs(e, c):
    """The case's host inputs for cell c: (x fp32, the four parameter tensors, eps_act, eps_b)."""
    S, B, K, N = e["shape"]
    xh = R.kind_x(e["kind"], B, K, S if e["x3d"] else 0)
    p = F.cell_params(c, N, K, lr=True)
    if e["eps"] == "memory":
        ea, eb = R.lr_eps(S, B, N, e.get("shift", 0))
    elif e["eps"] == "philox":
        ea, eb = R.philox_eps(SEED, LAYER_ID, OFFSET, S, B, N)
    else:
        ea = eb = None
    return xh, p, ea, eb


def _run(e, c, dev, plan_only=False):
    S, B, K, N = e["shape"]
    xh, p, ea, eb = _inputs(e, c)
    d = [_up(a, dev) for a in p]
    xf = _up(xh, dev)
    x = xf.to(BF) if e["xdt"] == "bf16" else xf
    ybf = e["ydt"] == "bf16"
    kw = dict(n_samples=S, sigma_p=1.0, math_mode=MATH[e["math"]], relu=e["relu"], y_dtype=BF if ybf else torch.float32, seed=SEED,
              layer_id=LAYER_ID, sample_offset=OFFSET, want_kl=False,
              eps_mode={"memory": L.EPS_MEMORY, "philox": L.EPS_PHILOX, "zero": L.EPS_ZERO}[e["eps"]])
    if e["eps"] == "memory":
        kw.update(eps_act=_up(ea, dev), eps_b=_up(eb, dev))
    ref_kw = dict(math=e["math"], relu=e["relu"], y_bf16=ybf, n_samples=S)
    gemm = e["form"] == G
    if gemm:
        kw["x_sq"] = (xf * xf).to(BF) if e["math"] == "bf16x3" else (x.float() * x.float()).to(BF)
        ref_kw["x_sq"] = kw["x_sq"]
        if e["math"] == "bf16x3":
            kw["x_lo"] = (xf - x.float()).to(BF)
            ref_kw["x_lo"] = kw["x_lo"]
    else:                                                     # the tile forms: every by-product lr_epilogue_item has
        kw.update(want_v=True, want_hfac=True, want_y16=not ybf)
    if e.get("final"):
        kw.update(want_hfac=False, want_y16=False)
    else:
        kw.update(form=e["form"], out_sq=torch.empty((S, B, N), dtype=BF, device=dev))
    if e["prepared"]:
        kw["w_frag"], kw["workspace"] = ops.lr_prepare(*d, x3=e["math"] == "bf16x3")
        kw["want_kl"] = True
    if e["scratch"]:
        kw["split_scratch"] = ops.lr_split_scratch_cached(1 if (not e["x3d"] and S > 1) else S, B, N, dev)
    if plan_only:
        return ops.lr_plan(x, *d, **kw)
    if e.get("final"):
        out = _final(e, x, d, kw, dev)
    else:
        out = ops.lr_linear_fwd(x, *d, **kw)
    ref = R.lr_ref(x if e["xdt"] == "bf16" else xh, *p, ea, eb, **ref_kw)
    return Launch(out, ref)


def _final(e, x, d, kw, dev):
    """bnn_lr_final_fwd on a classification target: the one-launch form K3r reads the layer's KL workspace (prepared) or does not
    touch it (parked), the two-launch form would have K3a rewrite it tile by tile -- its bits coming back unchanged is the proof."""
    S, B, K, N = e["shape"]
    assert N <= 16 and B <= 128 and K % 8 == 0 and K <= 2048 and S <= (4096 if e["prepared"] else 16)      # bnn_lr_final_fwd's `rows`
    ws = kw.get("workspace")
    if ws is None:
        ws = ops.lr_workspace(N, dev)
        ws.fill_(-7.0)
    before = ws.clone()
    target = torch.arange(B, device=dev) % N
    layer, fin = ops.lr_final_fwd((x,) + tuple(d), dict(kw, workspace=ws, want_kl=True, want_v=True),
                                  dict(workspaces=[ws], layer_in=[K], layer_out=[N], local_reparam=True, prior=ops.PriorSpec(False, 1.0),
                                       n_samples=S, target=target, mode="classification", scratch=ops.final_scratch(S, dev),
                                       ticket=torch.zeros(1, dtype=torch.int32, device=dev) if S > 1 else None))
    assert torch.equal(ws.view(torch.int32), before.view(torch.int32)), "bnn_lr_final_fwd took the two-launch form"
    return layer


def _np(t):
    return None if t is None else t.float().cpu().numpy()


def _sq_of_rounded(y):
    r = y.to(BF).float()
    return (r * r).to(BF)


def _judge(t, e, c, run):
    """Every element of every output of one launch, by the cell's regime."""
    out, ref = run
    y, v, hfac = _np(out["y"]), _np(out.get("v")), _np(out.get("hfac"))
    where = c.name
    if c.rho == 89.0:                                         # sigma = +inf; a ReLU turns NaN and -inf into 0
        for name, a in (("y", y), ("hfac", hfac), ("v", v)):
            if a is not None:
                assert np.all(~np.isfinite(a) | (a == 0)), (t.what, where, name)
        assert e["relu"] or not np.isfinite(y).any(), (t.what, where, "y")
        assert v is None or not np.isfinite(v).any(), (t.what, where, "v")
    elif c.tag != "regular":                                  # sigma = 0: rho = -200, and the band rho = -100
        for name, a in (("v", v), ("hfac", hfac)):
            if a is not None:
                assert np.all(a == 0), (t.what, where, name)
        sh = F.share(y, ref.y_mean, ref.b_y_mean)
        assert sh <= 1.0, (t.what, where, "y against m + b_mu", sh)
        if c.rho == F.RHO_BAND:
            t.note("y", False)
    else:
        if e["eps"] == "zero":
            t.add("y", F.share(y, ref.y_mean, ref.b_y_mean), where)
        t.add("y", F.share(y, ref.y, ref.b_y), where)
        if v is not None:
            t.add("v", F.share(v, ref.v, ref.b_v), where)
        if hfac is not None:
            t.add("hfac", F.share(hfac, ref.hfac, ref.b_hfac), where)
        if e["kind"] == "b" and v is not None:                 # the all-zero row
            assert np.all(v[:, 1] == 0) and np.all(hfac[:, 1] == 0), (t.what, where)
        if e["kind"] == "c" and v is not None:                 # what the device made of the underflowing squares
            t.band.setdefault("v", set()).add("0" if np.all(v == 0) else f"not 0 at rho {c.rho:g}")
        if out.get("y_lo") is not None:                        # split-bf16 planes: their sum is the fp32 y to 2^-16
            both = y.astype(np.float64) + _np(out["y_lo"])
            b = (ref.b_y - R.HALF_BF16 * np.abs(ref.y)) / (1 + R.HALF_BF16)                 # the bound before the bf16 term
            t.add("y+y_lo", F.share(both, ref.y, b + 2.0 ** -16 * (np.abs(ref.y) + b)), where)
    # exact functions of the launch's own y, in every cell
    if out.get("y16") is not None:
        assert _same(out["y16"], out["y"].to(BF)), (t.what, where, "y16")
    if out.get("y_sq") is not None:
        if e["math"] == "bf16x3" and e["ydt"] == "f32":         # this mode squares the fp32 y
            assert _same(out["y_sq"], (out["y"] * out["y"]).to(BF)), (t.what, where, "y_sq")
        elif e["math"] == "bf16x3":                              # ... which the planes give back to 2^-16: 2^-15 of the square + its rounding
            if c.tag == "regular":
                s = (out["y"].double() + out["y_lo"].double()) ** 2
                assert bool(((out["y_sq"].double() - s).abs() <= (2.0 ** -8 + 2.0 ** -14) * s).all()), (t.what, where, "y_sq")
        else:
            assert _same(out["y_sq"], _sq_of_rounded(out["y"])), (t.what, where, "y_sq")


def _same(a, b):
    """Bitwise equal bf16 tensors; NaN matches NaN whatever its payload."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(na, nb)) and bool(torch.equal(a.view(torch.int16)[~na], b.view(torch.int16)[~nb]))


@pytest.mark.parametrize("name", list(CASES))
def test_lr_forward_cell_by_cell(dev, name):
    e = CASES[name]
    t = Tally(name)
    cs = R.cells(e["grid"])
    if e["plan"] is not None:
        plan = _run(e, cs[0], dev, plan_only=True)
        assert {k: plan[k] for k in e["plan"]} == e["plan"], (name, plan)
    for c in cs:
        _judge(t, e, c, _run(e, c, dev))
    t.report()


@pytest.mark.parametrize("math", ["f32", "bf16"])
def test_module_eval_path(dev, monkeypatch, math):
    """BayesianLinearLR in eval mode with sample=False: y = x . M + b_mu (BNN_EPS_ZERO through the module), in both math modes."""
    import bnn_hip.runtime
    import networks
    B, K, N = 9, 33, 21
    monkeypatch.setattr(bnn_hip.runtime.state, "math", MATH[math])
    layer = networks.BayesianLinearLR(K, N, [-0.2, 0.2], [-5, -4], [1.0]).to(dev).eval()
    t = Tally(f"module sample=False {math}")
    x = R.kind_x("a", B, K)
    for c in R.cells("rho"):
        p = F.cell_params(c, N, K, lr=True)
        with torch.no_grad():
            for dst, src in zip((layer.weight_mu, layer.weight_rho, layer.bias_mu, layer.bias_rho), p):
                dst.copy_(_up(src, dev))
            y = layer(_up(x, dev), sample=False).cpu().numpy()
        ref = R.lr_ref(x, *p, None, None, math=math)
        if c.rho == 89.0:
            assert not np.isfinite(y).any(), c.name
        else:
            t.add("y", F.share(y, ref.y_mean[0], ref.b_y_mean[0]), c.name)
    t.report()


# ------------------------------------------------------------------------------------------------- the measured constant
def test_sqrt_error_constant(dev):
    """E_SQRT of tests/lr_fwd_ref.py, re-measured: a 1 x 1 layer with M = 0, b_mu = 0, sigma_b eps_b = 0 and eps_act = 1 returns
    y = fma(sqrt(v), 1, 0) + 0, the raw square root of the v it saves, bit for bit."""
    x = R.sqrt_probe_x()
    n = x.size
    one = lambda v: torch.full((1,), float(v), device=dev)
    rho = float(np.log(np.expm1(1.0)))
    out = ops.lr_linear_fwd(_up(x.reshape(n, 1), dev), one(0).view(1, 1), one(rho).view(1, 1), one(0), one(-200.0), n_samples=1, sigma_p=1.0,
                            math_mode=L.MATH_F32, relu=False, y_dtype=torch.float32, eps_mode=L.EPS_MEMORY,
                            eps_act=torch.ones((1, n, 1), device=dev), eps_b=torch.zeros((1, 1), device=dev), want_kl=False, want_v=True,
                            form=L.FORM_TILE)
    y, v = out["y"].cpu().numpy().ravel(), out["v"].cpu().numpy().ravel()
    assert np.all(v > 0) and np.all(np.abs(v / (x.astype(np.float64) ** 2) - 1) < 1e-5)
    e = R.sqrt_error_in_u(y, v)
    print(f"v_sqrt_f32 over v in 2^[-40, 40]: largest relative error {e:.4f} u (recorded {R.E_SQRT_MEASURED}, E_SQRT = {R.E_SQRT})")
    assert e <= R.E_SQRT / 2, e
