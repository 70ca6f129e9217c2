"""The correlation aggregates on device-resident arrays: device-event time per call, min / median / max over the repetitions.
One JSON line per measurement, appended to --out.

    python scripts/cor_bench.py [--reps 5] [--groups 100000] [--rows 100] [--large 200000] [--out FILE]

Reports the groups per second of --groups groups of --rows rows for each method (Pearson also as bytes per second: it reads x and
y twice, 32 bytes per row, the second time from cache where the group fits), and the time of one Kendall group of --large rows
(the large path: a sort in global memory, then the pair count over the whole device), with the pairs per second, next to Spearman
on the same group, which is that path without the pair count."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("anofox-statistics_amd")

METHODS = (("pearson", 0), ("spearman", 1), ("kendall", 2))


def time_call(ctx, off, x, y, method, reps, warm=2):
    times = []
    for r in range(reps + warm):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ctx.cor_batch_device(off, x, y, method)
        b.record()
        torch.cuda.synchronize()
        if r >= warm:
            times.append(a.elapsed_time(b))
    return float(np.min(times)), float(np.median(times)), float(np.max(times))


def emit(row, out):
    line = json.dumps(row)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--groups", type=int, default=100000)
    ap.add_argument("--rows", type=int, default=100)
    ap.add_argument("--large", type=int, default=200000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    ctx = pkg.Context(0)
    gen = torch.Generator(device=dev).manual_seed(1)
    n = args.groups * args.rows
    x = torch.randn(n, dtype=torch.float64, device=dev, generator=gen)
    y = 0.5 * x + torch.randn(n, dtype=torch.float64, device=dev, generator=gen)
    off = torch.arange(args.groups + 1, dtype=torch.int64, device=dev) * args.rows
    for name, m in METHODS:
        lo, med, hi = time_call(ctx, off, x, y, m, args.reps)
        row = {"method": name, "groups": args.groups, "rows": args.rows, "ms": {"min": round(lo, 4), "median": round(med, 4), "max": round(hi, 4)},
               "groups_per_s": round(args.groups / (med * 1e-3))}
        if m == 0:
            row["gbps_32B_per_row"] = round(32 * n / (med * 1e-3) / 1e9, 1)
        emit(row, args.out)
    if args.large > 0:
        L = args.large
        xl = torch.randn(L, dtype=torch.float64, device=dev, generator=gen)
        yl = 0.5 * xl + torch.randn(L, dtype=torch.float64, device=dev, generator=gen)
        offl = torch.tensor([0, L], dtype=torch.int64, device=dev)
        # Spearman on the same group: the large path without the pair count (compaction, two sorts, the runs, the moments)
        lo, med, hi = time_call(ctx, offl, xl, yl, 1, max(2, args.reps // 2), warm=1)
        emit({"method": "spearman", "groups": 1, "rows": L, "ms": {"min": round(lo, 3), "median": round(med, 3), "max": round(hi, 3)}}, args.out)
        lo, med, hi = time_call(ctx, offl, xl, yl, 2, max(2, args.reps // 2), warm=1)
        emit({"method": "kendall", "groups": 1, "rows": L, "ms": {"min": round(lo, 3), "median": round(med, 3), "max": round(hi, 3)},
              "pairs_per_s": round(L * (L - 1) / 2 / (med * 1e-3))}, args.out)
    ctx.close()


if __name__ == "__main__":
    main()
