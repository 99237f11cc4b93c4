#!/usr/bin/env python3
"""Bit-level record of everything that draws epsilon: sha256 digests of the raw bytes of a fixed set of launches.

The epsilon map (include/bnn_hip.h) is frozen, and the block GEMM K1b2 promises outputs bit for bit; a change to the
generator's instructions (Philox rounds, Box-Muller) or to K1b2's loop, prologue or epilogue must not move one bit.  This
file defines the launches (`cases`) and is both
  * the recorder: run against the library of the commit to compare with (BNN_HIP_LIB=<that commit's libbnn_hip.so>), it
    writes tests/golden/k1b2_parent_digests.json;
  * the case list of tests/test_gpu_epsilon_bits.py, which recomputes every case with the built library.
Inputs come from CPU generators (and sigma = log1p(exp(rho)) from the CPU), so a digest depends on the library alone.

usage (GPU box):  BNN_HIP_LIB=/path/to/parent/libbnn_hip.so python tools/epsilon_bits.py
"""
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(REPO, "bayesian-neural-network_amd"), REPO):
    if _p not in sys.path:
        sys.path.insert(0, _p)
GOLDEN = os.path.join(REPO, "tests", "golden", "k1b2_parent_digests.json")

PHILOX_CASES = [(0, 0, 2, 5, 37), (9, 1000, 1, 16, 8), (4, 0, 1, 130, 1201)]            # (tensor id, first sample, S, rows, cols)
# (pairs, B, K, N) of the block form K1b2.  (5, 128, 64, 80): five tiles -- group 1 is one real wave and three phantom waves --
# and an odd pair count (an idle pair slot); (4, 20, 72, 72): a half-real tile and three phantom waves, a partial k-step on the
# clamped staging path, 20 of a block's 128 rows; the two hidden layers of the benchmark's network.
BLOCK_SHAPES = [(5, 128, 64, 80), (4, 20, 72, 72), (6, 128, 784, 1200), (6, 128, 1200, 1200)]
OTHER_SHAPE = (3, 20, 72, 37)                                                            # the tile form K1a and the sampler K1s


def case_names():
    names = [f"philox_normal-{'-'.join(map(str, c))}" for c in PHILOX_CASES]
    for sh in BLOCK_SHAPES:
        for math in ("bf16", "bf16x3"):
            for relu in (0, 1):
                for y in ("bf16", "f32"):
                    names.append(f"k1b2-{'-'.join(map(str, sh))}-{math}-relu{relu}-y{y}")
    return names + ["k1a-" + "-".join(map(str, OTHER_SHAPE)), "k1s-" + "-".join(map(str, OTHER_SHAPE)), "graphed_elbo-g4-s1"]


def digest(t):
    """sha256 of a tensor's raw bytes (bf16 through its 16-bit patterns)."""
    import torch
    t = t.detach().contiguous().cpu()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


def _layer(S, B, K, N, dev):
    import torch
    gen = torch.Generator(device="cpu").manual_seed(K * 131 + N * 7 + S)
    x = torch.rand(S, B, K, generator=gen) - 0.25
    wm = (torch.rand((N, K), generator=gen) - 0.5) * 0.4
    wr = torch.rand((N, K), generator=gen) - 5.0
    bm = (torch.rand(N, generator=gen) - 0.5) * 0.4
    br = torch.rand(N, generator=gen) - 5.0
    sig = torch.log1p(torch.exp(wr))
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return tuple(a.to(dev) for a in (hi, lo, wm, wr, bm, br, sig))


def run_case(name, dev):
    """{tensor name: digest} of one case, computed with the loaded library."""
    import torch
    import bnn_hip
    from bnn_hip import ops, _lib as L
    kind, _, rest = name.partition("-")
    if kind == "philox_normal":
        tid, s0, S, rows, cols = map(int, rest.split("-"))
        return {"eps": digest(ops.philox_normal(2026, tid, s0, S, rows, cols, dev))}
    if kind == "k1b2":
        f = rest.split("-")
        S, B, K, N = map(int, f[:4])
        x3, relu, ydt = f[4] == "bf16x3", f[5] == "relu1", torch.bfloat16 if f[6] == "ybf16" else torch.float32
        hi, lo, wm, wr, bm, br, sig = _layer(S, B, K, N, dev)
        kw = dict(n_samples=S, prior=ops.PriorSpec(False, 0.9), math_mode=L.MATH_BF16X3 if x3 else L.MATH_BF16, relu=relu, y_dtype=ydt,
                  eps_mode=L.EPS_PHILOX, seed=78, layer_id=1, sample_offset=11, want_stats=True, want_scalars=True, form=L.FORM_GEMM,
                  w_sigma=sig, dump_eps=True)
        if x3:
            kw["x_lo"] = lo
        plan = ops.bbb_plan(hi, wm, wr, bm, br, **kw)
        assert plan["form"] == L.FORM_GEMM and plan["waves"] == 8, plan
        out = ops.bbb_linear_fwd(hi, wm, wr, bm, br, **kw)
        d = {k: digest(out[k]) for k in ("y", "eps_w", "eps_b", "log_prior", "log_q")}
        if out.get("y_lo") is not None:
            d["y_lo"] = digest(out["y_lo"])
        return d
    if kind in ("k1a", "k1s"):
        S, B, K, N = map(int, rest.split("-"))
        hi, lo, wm, wr, bm, br, sig = _layer(S, B, K, N, dev)
        if kind == "k1a":
            kw = dict(n_samples=S, prior=ops.PriorSpec(False, 0.9), math_mode=L.MATH_BF16, relu=True, y_dtype=torch.float32,
                      eps_mode=L.EPS_PHILOX, seed=78, layer_id=2, sample_offset=3, want_stats=True, want_scalars=True, form=L.FORM_TILE,
                      dump_eps=True)
            assert ops.bbb_plan(hi, wm, wr, bm, br, **kw)["form"] == L.FORM_TILE
            out = ops.bbb_linear_fwd(hi, wm, wr, bm, br, **kw)
            return {k: digest(out[k]) for k in ("y", "eps_w", "eps_b", "log_prior", "log_q")}
        res = ops.bbb_sample_weights([dict(w_mu=wm, w_rho=wr, b_mu=bm, b_rho=br, prior=ops.PriorSpec(False, 0.9), layer_id=2)],
                                     n_samples=S, seed=78, sample_offset=3)[0]
        return {"w": digest(res["w"]), "b": digest(res["b"])}
    if kind == "graphed_elbo":
        import numpy as np
        import networks
        from bnn_hip import engine, synth
        G, S, B, dims = 4, 1, 128, (784, 1200, 10)
        bnn_hip.set_math("bf16")
        mp = dict(input_shape=dims[0], classes=dims[2], batch_size=B, hidden_units=dims[1], mode="classification", mu_init=[-0.2, 0.2],
                  rho_init=[-5, -4], prior_init=[1.0], mixture_prior=False, local_reparam=False)
        net = networks.BayesianNetwork(mp)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_state_dict(*dims, False).items()})
        net.to(dev).train()
        xs, ys = zip(*[synth.synth_batch("classification", B, dims[0], dims[2], seed=100 + m) for m in range(G)])
        bnn_hip.manual_seed(5, counter=300)
        ev = engine.GraphedElbo(net, torch.from_numpy(np.stack(xs)).to(dev), torch.from_numpy(np.stack(ys)).to(dev), S, stacked=True)
        sums = ev.replay().clone()
        torch.cuda.synchronize()
        d = {"sums": digest(sums), "logits": digest(ev.logits)}
        d.update({"out." + k: digest(v) for k, v in sorted(ev.out.items())})
        bnn_hip.manual_seed(2026)
        return d
    raise KeyError(name)


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
