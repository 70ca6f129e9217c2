"""The rank test aggregates on device-resident arrays: device-event time per call, min / median / max over the repetitions.  One
JSON line per measurement, appended to --out (default profiles/rank_test_bench.jsonl).

    python scripts/rank_test_bench.py [--reps 5] [--groups 100000] [--rows 100,1000] [--large 200000] [--out FILE]

Reports the groups per second of --groups groups (at 1000 rows a tenth of them, the same number of rows) for Mann-Whitney, Wilcoxon
signed-rank and Kruskal-Wallis (three samples), and spearman_agg's kernels in the same run on the same shapes as the yardstick: it
sorts each group twice, Mann-Whitney and Wilcoxon once.  Then one group of --large rows (the large path) for all four."""
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

TESTS = (("mann_whitney", 0), ("wilcoxon", 1), ("kruskal_wallis", 2))


def time_call(fn, reps, warm=2):
    times = []
    for r in range(reps + warm):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if r >= warm:
            times.append(a.elapsed_time(b))
    return float(np.min(times)), float(np.median(times)), float(np.max(times))


def emit(row, out):
    line = json.dumps(row)
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")


def shape(ctx, dev, gen, groups, rows, reps, warm, out):
    n = groups * rows
    v = torch.randn(n, dtype=torch.float64, device=dev, generator=gen)
    y = 0.5 * v + torch.randn(n, dtype=torch.float64, device=dev, generator=gen)
    sample = torch.randint(0, 2, (n,), dtype=torch.int32, device=dev, generator=gen)
    sample3 = torch.randint(0, 3, (n,), dtype=torch.int32, device=dev, generator=gen)
    off = torch.arange(groups + 1, dtype=torch.int64, device=dev) * rows
    calls = [(name, (lambda t=t: ctx.rank_test_batch_device(off, v, y if t == 1 else None, None if t == 1 else (sample3 if t == 2 else sample), t)))
             for name, t in TESTS]
    calls.append(("spearman", lambda: ctx.cor_batch_device(off, v, y, 1)))
    for name, fn in calls:
        lo, med, hi = time_call(fn, reps, warm)
        emit({"method": name, "groups": groups, "rows": rows, "ms": {"min": round(lo, 4), "median": round(med, 4), "max": round(hi, 4)},
              "groups_per_s": round(groups / (med * 1e-3))}, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--groups", type=int, default=100000)
    ap.add_argument("--rows", default="100,1000")
    ap.add_argument("--large", type=int, default=200000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_test_bench.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    ctx = pkg.Context(0)
    gen = torch.Generator(device=dev).manual_seed(1)
    first = None
    for rows in (int(r) for r in args.rows.split(",")):
        first = rows if first is None else first
        shape(ctx, dev, gen, max(1, args.groups * first // rows), rows, args.reps, 2, args.out)
    if args.large > 0:
        shape(ctx, dev, gen, 1, args.large, max(2, args.reps // 2), 1, args.out)
    ctx.close()


if __name__ == "__main__":
    main()
