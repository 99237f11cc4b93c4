#!/usr/bin/env python3
"""F11: the time of one PosteriorStats.update() -- the twelve histograms of write_weight_histograms -- at ClassConfig
(784-1200-1200-10) and RegConfig (1-400-400-1), beside
  (a) the same records built from torch ops on the same device, per tensor: transform, min, max, sum, sum of squares,
      torch.bucketize + torch.bincount against the same edges (no host read inside the window);
  (b) the reference's route, per tensor: .cpu() + np.histogram (utils/logger_utils.py:13-26 through add_histogram);
  (c) the time to read the parameters once at the measured HBM rate (6.29 TB/s, float4 copy).
The three device figures alternate in one process (update, torch, update, torch, ...), each window is `--iters` calls
between two device events after `--warmup` calls, and the median and spread of `--rounds` windows are reported; the
update is also timed as a replayed graph.  (b) is a host clock around work that ends in the copy.  Results are checked
against each other before anything is timed.  One JSON line; --out also writes it to a file.
usage: python tools/posterior_stats_bench.py [--iters 200] [--rounds 7] [--out results/posterior_stats_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "bayesian-neural-network_amd"))

import numpy as np   # noqa: E402
import torch         # noqa: E402

HBM_GBS = 6290.0
CONFIGS = {"ClassConfig": dict(input_shape=784, hidden_units=1200, classes=10, mode="classification"),
           "RegConfig": dict(input_shape=1, hidden_units=400, classes=1, mode="regression")}


def build(cfg, dev):
    import networks
    torch.manual_seed(0)
    net = networks.BayesianNetwork(dict(cfg, batch_size=128, mu_init=[-0.2, 0.2], rho_init=[-5, -4], prior_init=[1.0],
                                        mixture_prior=False, local_reparam=False)).to(dev)
    with torch.no_grad():                                   # a trained posterior's spread: mu over ~30 bins, sigma over ~10
        for l in (net.l1, net.l2, net.l3):
            l.weight_mu.normal_(0.0, 0.05)
            l.weight_rho.uniform_(-5.5, -4.5)
    return net


def tensors(net):
    out = []
    for which in ("weight", "bias"):
        for l in (net.l1, net.l2, net.l3):
            out += [(getattr(l, which + "_mu").detach(), False), (getattr(l, which + "_rho").detach(), True)]
    return out


def torch_route(ts, edges_dev):
    """(a): per tensor the transform, the four moments and the counts, all on the device."""
    nb = edges_dev.numel() - 1
    out = []
    for t, is_rho in ts:
        v = torch.log1p(torch.exp(t)) if is_rho else t
        v = v.reshape(-1)
        d = v.double()
        idx = torch.bucketize(d, edges_dev, right=True) - 1
        idx = torch.where(d == edges_dev[-1], torch.full_like(idx, nb - 1), idx)
        inside = (idx >= 0) & (idx < nb)
        counts = torch.bincount(idx[inside], minlength=nb)
        out.append((counts, v.min(), v.max(), d.sum(), (d * d).sum()))
    return out


def host_route(ts, edges):
    """(b): the reference's add_histogram per tensor: a device-to-host copy and np.histogram."""
    out = []
    for t, is_rho in ts:
        v = (torch.log1p(torch.exp(t)) if is_rho else t).cpu().numpy().reshape(-1)
        out.append(np.histogram(v.astype(np.float64), bins=edges)[0])
    return out


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters                  # us per call


def spread(xs):
    return {"median_us": round(statistics.median(xs), 3), "min_us": round(min(xs), 3), "max_us": round(max(xs), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("posterior_stats_bench: needs a ROCm device (no CPU timing stands in for it)")
    from bnn_hip import diagnostics as D
    dev = torch.device("cuda:0")
    edges = D.tensorboard_bins()
    edges_dev = torch.from_numpy(edges).to(dev)
    result = {"tool": "posterior_stats_bench", "iters": args.iters, "rounds": args.rounds, "hbm_GBs": HBM_GBS, "configs": {}}
    for name, cfg in CONFIGS.items():
        net = build(cfg, dev)
        ts = tensors(net)
        ps = D.PosteriorStats(net, bins=edges)
        n_params = sum(t.numel() for t, _ in ts)
        # the three routes agree before anything is timed (sigma by torch's log1p(exp) may differ from the kernel's
        # softplus in the last place: a handful of elements may sit in the neighbouring bin)
        ps.update()
        raw = ps.raw()
        tor = torch_route(ts, edges_dev)
        hst = host_route(ts, edges)
        moved = 0
        for (tag, r), (c, *_), h in zip(raw.items(), tor, hst):
            assert np.array_equal(c.cpu().numpy(), h), tag
            moved += int(np.abs(r["counts"] - h).sum()) // 2
            assert int(r["counts"].sum()) == int(h.sum()), tag
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ps.update()
        routes = {"update": ps.update, "update_graph": g.replay, "torch_ops": lambda: torch_route(ts, edges_dev)}
        for fn in routes.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in routes}
        for _ in range(args.rounds):                        # alternating, in one process
            for k, fn in routes.items():
                times[k].append(window(fn, args.iters))
        host = []
        for _ in range(max(3, args.rounds)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host_route(ts, edges)
            host.append((time.perf_counter() - t0) * 1e6)
        floor_us = 4.0 * n_params / (HBM_GBS * 1e9) * 1e6
        entry = {k: spread(v) for k, v in times.items()}
        entry["host_numpy"] = spread(host)
        entry.update(parameters=n_params, bytes_read=4 * n_params, hbm_floor_us=round(floor_us, 3),
                     elements_in_a_neighbouring_bin_vs_numpy=moved,
                     update_over_hbm_floor=round(entry["update_graph"]["median_us"] / floor_us, 2),
                     torch_ops_over_update=round(entry["torch_ops"]["median_us"] / entry["update"]["median_us"], 2),
                     host_numpy_over_update=round(entry["host_numpy"]["median_us"] / entry["update"]["median_us"], 2))
        result["configs"][name] = entry
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
