"""K5 measurement: MC-dropout prediction of MLP_Dropout, one variant after the other in the same process, device-event
timings after warm-up (median of the repeats):
  - reference: torch MLP_Dropout with enable_dropout(), S forward passes one after the other + the softmax mean
    (classification/class_task.py:230-236) or the stacked outputs (regression/reg_task.py:186-195);
  - eager predict_mc (classification) / predictive with 5 quantiles (regression): one launch per layer + the summary;
  - predictive_graph replay.
Shapes: 784-1200-1200-10 at B = 128 for S = 10, 64, 256; the 10 000-row test set at S = 10; regression 1-400-400-1 at
B = 400, S = 10, 5 quantiles.  Prints one line per case, then the rows as JSON.
usage: python tools/mc_dropout_bench.py [--math bf16|f32]
       python tools/mc_dropout_bench.py --profile-run      (the 10 000-row evaluation only, 20 times; run it under
                                                           rocprofv3 --kernel-trace --stats -d DIR -o run -- ...)
       python tools/mc_dropout_bench.py --stats DIR/run_results.db | FILE_kernel_stats.csv [--math bf16|f32]
                                                          (the layer-2 kernel's TF/s from that run: 2 S B H^2 / time;
                                                           rocprofv3's database, or its csv output with -f csv)"""
import argparse
import csv
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "bayesian-neural-network_amd"))
sys.path.insert(0, REPO)

PEAK_TF = {"bf16": 2500.0, "f32": 157.3}    # MI355X dense matrix-core peaks: bf16, and the fp32-input MFMA rate
TEST_ROWS, H = 10000, 1200


def layer2_tflops(stats_path, math):
    """TF/s of the hidden-to-hidden launch of the 10 000-row evaluation from a rocprofv3 kernel_stats.csv."""
    if stats_path.endswith(".db"):
        import sqlite3
        db = sqlite3.connect(stats_path)
        rows = [dict(Name=n, Calls=str(c), AverageNs=str(a), TotalDurationNs=str(t)) for n, c, a, t in
                db.execute("select name, count(*), avg(end - start), sum(end - start) from kernels group by name")]
    else:
        rows = list(csv.DictReader(open(stats_path)))
    # layer 2 is the only launch with bf16 activations in and out (bf16 math), or the fp32 kernel's middle launch
    dense = [r for r in rows if "dense_fwd_kernel" in r["Name"]]
    for r in dense:
        print(f"{r['Name'][:110]:110s} calls {r['Calls']:>5s} avg {float(r['AverageNs']) / 1e3:9.1f} us")
    if math == "bf16":
        pick = [r for r in dense if r["Name"].count("__bf16") == 3 or "IDF16bDF16bDF16b" in r["Name"]]
        avg_ns = float(pick[0]["AverageNs"])
    else:   # f32: the three layers share one instantiation; layer 2 dominates -- report the total over the calls / 3 layers
        pick = dense[:1]
        avg_ns = float(pick[0]["TotalDurationNs"]) / float(pick[0]["Calls"])
    flop = 2.0 * 10 * TEST_ROWS * H * H
    tf = flop / avg_ns / 1e3
    out = dict(kernel=pick[0]["Name"][:80], avg_us=avg_ns / 1e3, tflops=tf, peak_tflops=PEAK_TF[math], fraction=tf / PEAK_TF[math])
    print(json.dumps(out))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--math", default="bf16", choices=("bf16", "f32"))
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--stats")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if args.stats:
        layer2_tflops(args.stats, args.math)
        return

    import torch
    import bnn_hip
    import networks

    dev = torch.device("cuda:0")
    bnn_hip.set_math(args.math)

    def mlp_of(inp, hid, out, mode):
        torch.manual_seed(0)
        m = networks.MLP_Dropout(dict(input_shape=inp, classes=out, batch_size=128, hidden_units=hid, mode=mode)).to(dev)
        m.eval()
        m.enable_dropout()
        return m

    def timed(fn, reps):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        return statistics.median(ts)

    g = torch.Generator().manual_seed(1)
    if args.profile_run:
        mlp = mlp_of(784, H, 10, "classification")
        x = torch.rand((TEST_ROWS, 1, 28, 28), generator=g).to(dev)
        with torch.no_grad():
            for _ in range(args.reps):
                mlp.predict_mc(x, 10)
        torch.cuda.synchronize()
        return

    rows = []

    def report(case, form, us):
        rows.append(dict(case=case, form=form, math=args.math, us=us))
        print(f"{case:40s} {form:28s}: {us:10.1f} us", flush=True)

    cases = [("784-1200-1200-10 B128", 128, S) for S in (10, 64, 256)] + [("784-1200-1200-10 test set", TEST_ROWS, 10)]
    with torch.no_grad():
        for name, B, S in cases:
            mlp = mlp_of(784, H, 10, "classification")
            x = torch.rand((B, 1, 28, 28), generator=g).to(dev)
            case = f"{name} S{S}"
            reps = args.reps if B * S <= 20000 else max(3, args.reps // 4)
            report(case, "reference loop", timed(lambda: torch.stack([torch.softmax(mlp(x), -1) for _ in range(S)]).mean(0), reps))
            report(case, "predict_mc (eager)", timed(lambda: mlp.predict_mc(x, S), reps))
            pg = mlp.predictive_graph(x, S)
            report(case, "predictive_graph replay", timed(pg.replay, reps))
            del pg
        mlp = mlp_of(1, 400, 1, "regression")
        x = torch.randn((400, 1), generator=g).to(dev)
        q = (0.05, 0.25, 0.5, 0.75, 0.95)
        case = "1-400-400-1 B400 S10 5 quantiles"
        report(case, "reference loop", timed(lambda: torch.stack([mlp(x) for _ in range(10)]), args.reps))
        report(case, "predictive (eager)", timed(lambda: mlp.predictive(x, 10, quantiles=q), args.reps))
        pg = mlp.predictive_graph(x, 10, quantiles=q)
        report(case, "predictive_graph replay", timed(pg.replay, args.reps))
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
