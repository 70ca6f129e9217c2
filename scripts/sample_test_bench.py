"""The sample test aggregates on device-resident arrays: device-event time per call, min / median / max over the repetitions.  One
JSON line per measurement, appended to --out (default profiles/sample_test_bench.jsonl).

    python scripts/sample_test_bench.py [--reps 5] [--groups 100000] [--rows 100,1000] [--large 200000] [--out FILE]

Reports the groups and rows per second of --groups groups (at 1000 rows a tenth of them, the same number of rows) for the Welch,
Student and paired t-test, Yuen, Fisher and Welch ANOVA and Brown-Forsythe (three arms) and Brunner-Munzel, and in the same run on
the same shapes the two yardsticks with their ratios: pearson_agg's kernels for the Welch t-test (both stream a group twice without
staging) and Mann-Whitney for Yuen and Brunner-Munzel (one sort against two and three).  Then one group of --large rows (the large
path; the t-test streams it by one wavefront) for all of them."""
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

# (name, test, options, the second column: y, two-arm ids or three-arm ids, the yardstick)
TESTS = (("t_welch", 0, {}, "two", "pearson"), ("t_student", 0, {"kind": "student"}, "two", "pearson"),
         ("t_paired", 0, {"kind": "paired"}, "y", "pearson"), ("yuen", 1, {}, "two", "mann_whitney"),
         ("anova", 2, {}, "three", None), ("anova_welch", 2, {"kind": "welch"}, "three", None), ("brown_forsythe", 3, {}, "three", None),
         ("brunner_munzel", 4, {}, "two", "mann_whitney"))


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
    ids = {"two": torch.randint(0, 2, (n,), dtype=torch.int32, device=dev, generator=gen),
           "three": torch.randint(0, 3, (n,), dtype=torch.int32, device=dev, generator=gen)}
    off = torch.arange(groups + 1, dtype=torch.int64, device=dev) * rows
    yard = {"pearson": time_call(lambda: ctx.cor_batch_device(off, v, y, 0), reps, warm)[1],
            "mann_whitney": time_call(lambda: ctx.rank_test_batch_device(off, v, None, ids["two"], 0), reps, warm)[1]}
    for name, med in yard.items():
        emit({"method": name, "groups": groups, "rows": rows, "ms": {"median": round(med, 4)}, "rows_per_s": round(n / (med * 1e-3))}, out)
    for name, test, opts, second, against in TESTS:
        o = pkg.parse_sample_test_options(opts, test)
        fn = (lambda: ctx.sample_test_batch_device(off, v, y, None, test, o)) if second == "y" else \
             (lambda: ctx.sample_test_batch_device(off, v, None, ids[second], test, o))
        lo, med, hi = time_call(fn, reps, warm)
        row = {"method": name, "groups": groups, "rows": rows, "ms": {"min": round(lo, 4), "median": round(med, 4), "max": round(hi, 4)},
               "groups_per_s": round(groups / (med * 1e-3)), "rows_per_s": round(n / (med * 1e-3))}
        if against:
            row["time_over_" + against] = round(med / yard[against], 3)
        emit(row, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--groups", type=int, default=100000)
    ap.add_argument("--rows", default="100,1000")
    ap.add_argument("--large", type=int, default=200000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_test_bench.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
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
