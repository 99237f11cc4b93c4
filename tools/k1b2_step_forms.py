#!/usr/bin/env python3
"""Bit-level record of the step bodies of the pair block GEMM K1b2: sha256 digests of the raw bytes of a fixed set of launches.

A wave of K1b2 picks the body of its k-step once, ahead of the loop (csrc/bbb_linear.hip: Gaussian prior without epsilon dump x
{no statistics, statistics, statistics + sum of log sigma} for maskless steps, one generic body for everything else, maskless or
masked, and the phantom wave's).  Whatever body runs, the bits of y, of the per-sample scalars and of the dumped epsilon are those of the commit
before the bodies existed.  This file defines the launches (`SHAPES`, `case_names`, `launch`) and is both
  * the recorder: run against the library of the commit to compare with (BNN_HIP_LIB=<that commit's libbnn_hip.so>), it writes
    tests/golden/k1b2_step_forms_parent.json;
  * the case list and launcher of tests/test_gpu_k1b2_step_forms.py, which recomputes every case with the built library.
Inputs come from CPU generators, sigma from the library's own softplus launch (K1b, which takes rho, forms the same values in its
registers), so a digest depends on the library alone.  The piece-order index maps are restated here from include/bnn_hip.h
(bnn_layout), not taken from the package.

usage (GPU box):  BNN_HIP_LIB=/path/to/parent/libbnn_hip.so python tools/k1b2_step_forms.py
"""
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(REPO, "bayesian-neural-network_amd"), REPO):
    if _p not in sys.path:
        sys.path.insert(0, _p)
GOLDEN = os.path.join(REPO, "tests", "golden", "k1b2_step_forms_parent.json")

# (pairs S, B, K, N)
SHAPES = [(4, 128, 64, 64),      # all full
          (5, 100, 40, 72),      # odd pair count, short batch, an 8-k tail step, a partial feature tile, phantom waves
          (4, 128, 784, 80),     # the first layer's tail of 16 k
          (3, 300, 72, 80)]      # three batch blocks per sample: a block holds a pair with statistics beside one without, and
                                 # sample 0's pair beside another sample's -- two step bodies across the same barriers
LAYOUTS = ("rows", "pieces")     # row-major operands | x, y and (mu, sigma) in piece order
PRIORS = ("gauss", "mixture")
TENSORS = ("y", "log_prior", "log_q", "eps_w", "eps_b")


def case_names():
    return [f"{'-'.join(map(str, sh))}-{lay}-{pr}" for sh in SHAPES for lay in LAYOUTS for pr in PRIORS]


def parse(name):
    f = name.split("-")
    return tuple(map(int, f[:4])), f[4], f[5]


def digest(t):
    """sha256 of a tensor's raw bytes (bf16 through its 16-bit patterns)."""
    import torch
    t = t.detach().contiguous().cpu()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


def to_pieces(x):
    """Host re-ordering of a row-major bf16 [S, B, K] tensor: the raw bits (int16) of the piece-order buffer, pads zero.
    [row][batch block of 128][k-step t][batch tile m][lane][8 bf16], lane (r = lane & 15, q = lane >> 4) of piece (t, m) holding
    x[128 block + 16 m + r][32 t + 8 q .. + 7]."""
    import numpy as np
    import torch
    rows, B, K = x.shape
    mbs, ks = (B + 127) // 128, (K + 31) // 32
    row = np.arange(rows, dtype=np.int64)[:, None, None]
    b = np.arange(B, dtype=np.int64)[None, :, None]
    k = np.arange(K, dtype=np.int64)[None, None, :]
    blk, m, r = b // 128, (b % 128) // 16, b % 16
    t, q, e = k // 32, (k % 32) // 8, k % 8
    idx = ((((row * mbs + blk) * ks + t) * 8 + m) * 64 + q * 16 + r) * 8 + e
    buf = np.zeros(rows * mbs * ks * 8 * 64 * 8, dtype=np.int16)
    buf[idx.reshape(-1)] = x.detach().cpu().contiguous().view(torch.int16).numpy().reshape(-1)
    return torch.from_numpy(buf)


def params_to_pieces(mu, sigma):
    """Host re-ordering of the row-major fp32 [N, K] (mu, sigma): the raw bits (int32) of the parameter pieces, pads zero.
    [feature tile T][k-step t][mu lo | mu hi | sigma lo | sigma hi][lane][4 fp32], lane (r, q) holding
    mu | sigma [16 T + r][32 t + 8 q + 0..3] (lo) and + 4..7 (hi)."""
    import numpy as np
    import torch
    N, K = mu.shape
    T, ks = (N + 15) // 16, (K + 31) // 32
    n = np.arange(N, dtype=np.int64)[:, None]
    k = np.arange(K, dtype=np.int64)[None, :]
    tile, r, t, q, h, e = n // 16, n % 16, k // 32, (k % 32) // 8, (k % 8) // 4, k % 4
    buf = np.zeros(T * ks * 4 * 64 * 4, dtype=np.int32)
    for first, src in ((0, mu), (2, sigma)):
        idx = ((((tile * ks + t) * 4 + first + h) * 64 + q * 16 + r) * 4 + e).reshape(-1)
        buf[idx] = src.detach().cpu().contiguous().view(torch.int32).numpy().reshape(-1)
    return torch.from_numpy(buf)


_inputs = {}


def inputs(shape, dev):
    """(x bf16 row-major, x in piece order, (w_mu, w_rho, b_mu, b_rho), sigma, (mu, sigma) in piece order), made once per shape."""
    import torch
    from bnn_hip import ops
    key = (shape, str(dev))
    if key not in _inputs:
        S, B, K, N = shape
        gen = torch.Generator(device="cpu").manual_seed(S * 1000 + B + K * 7 + N)
        x = (torch.rand(S, B, K, generator=gen) - 0.3).to(torch.bfloat16)
        wm = (torch.rand((N, K), generator=gen) - 0.5) * 0.4
        wr = torch.rand((N, K), generator=gen) - 5.0
        bm = (torch.rand(N, generator=gen) - 0.5) * 0.4
        br = torch.rand(N, generator=gen) - 5.0
        sig = ops.softplus(wr.to(dev))                    # the hoisted sigma as the library makes it: what K1b takes in its registers
        xp = ops.pieces_activation((S, B, K), dev)
        xp.view(torch.int16).view(-1).copy_(to_pieces(x).to(dev))
        wp = ops.param_pieces(N, K, dev)
        wp.view(torch.int32).view(-1).copy_(params_to_pieces(wm, sig).to(dev))
        _inputs[key] = (x.to(dev), xp, tuple(a.to(dev) for a in (wm, wr, bm, br)), sig, wp)
    return _inputs[key]


def prior_of(name):
    from bnn_hip import ops
    return ops.PriorSpec(True, 1.0, 0.5, 1.0, 0.05) if name == "mixture" else ops.PriorSpec(False, 0.9)


def launch(shape, layout, prior, dev, want_stats=True, dump_eps=True, hoisted=True):
    """One launch of the forced block form; `hoisted=False` is K1b (parameters in registers, row-major operands only).  Returns the
    result dict with y row-major.  A hoisted launch asserts from the plan that it is the 8-wave pair form K1b2."""
    import torch
    from bnn_hip import ops, _lib as L
    S, B, K, N = shape
    x, xp, w, sig, wp = inputs(shape, dev)
    pieces = layout == "pieces"
    assert hoisted or not pieces
    kw = dict(n_samples=S, prior=prior_of(prior), math_mode=L.MATH_BF16, relu=True, y_dtype=torch.bfloat16, eps_mode=L.EPS_PHILOX,
              seed=41, layer_id=1, sample_offset=3, want_stats=want_stats, want_scalars=want_stats, dump_eps=dump_eps,
              form=L.FORM_GEMM, w_sigma=sig if hoisted else None)
    if pieces:
        kw.update(out=ops.pieces_activation((S, B, N), dev), w_pieces=wp)
    xin = xp if pieces else x
    if hoisted:
        plan = ops.bbb_plan(xin, *w, **kw)
        assert plan["form"] == L.FORM_GEMM and plan["waves"] == 8, plan
    out = dict(ops.bbb_linear_fwd(xin, *w, **kw))
    if pieces:
        out["y"] = ops.unpiece(out["y"])
    return out


def run_case(name, dev):
    """{tensor name: digest} of one case, computed with the loaded library."""
    shape, layout, prior = parse(name)
    out = launch(shape, layout, prior, dev)
    return {k: digest(out[k]) for k in TENSORS}


def main():
    import torch
    from bnn_hip import _lib as L
    dev = torch.device("cuda:0")
    data = {name: run_case(name, dev) for name in case_names()}
    with open(GOLDEN, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(data)} cases from {L.LIB_PATH} -> {GOLDEN}")


if __name__ == "__main__":
    main()
