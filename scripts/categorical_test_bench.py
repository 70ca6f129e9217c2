"""The categorical test aggregates on device-resident arrays: device-event time per call, min / median / max over the repetitions.
One JSON line per measurement, appended to --out (default profiles/categorical_test_bench.jsonl).

    python scripts/categorical_test_bench.py [--reps 5] [--groups 100000] [--rows 100,1000,5000] [--out FILE]

Reports the groups and rows per second of --groups groups (at more rows per group fewer of them, the same number of rows) for the
chi-square test on 2 x 2 and on 5 x 7 labels and for Fisher's exact test, and in the same run on the same row counts the
Kruskal-Wallis test with the ratios to it: it and the chi-square test both compact a group and sort it twice."""
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

# (name, test, the levels of a and of b)
TESTS = (("chisq_2x2", 0, 2, 2), ("chisq_5x7", 0, 5, 7), ("fisher_exact", 2, 2, 2))


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
    ids = torch.randint(0, 3, (n,), dtype=torch.int32, device=dev, generator=gen)
    off = torch.arange(groups + 1, dtype=torch.int64, device=dev) * rows
    yard = time_call(lambda: ctx.rank_test_batch_device(off, v, None, ids, 2), reps, warm)[1]
    emit({"method": "kruskal_wallis", "groups": groups, "rows": rows, "ms": {"median": round(yard, 4)}, "rows_per_s": round(n / (yard * 1e-3))}, out)
    for name, test, r, c in TESTS:
        a = torch.randint(0, r, (n,), dtype=torch.int32, device=dev, generator=gen)
        b = (a + torch.randint(0, c, (n,), dtype=torch.int32, device=dev, generator=gen) * torch.randint(0, 2, (n,), dtype=torch.int32, device=dev, generator=gen)) % c
        lo, med, hi = time_call(lambda: ctx.categorical_test_batch_device(off, a, b, test), reps, warm)
        emit({"method": name, "groups": groups, "rows": rows, "ms": {"min": round(lo, 4), "median": round(med, 4), "max": round(hi, 4)},
              "groups_per_s": round(groups / (med * 1e-3)), "rows_per_s": round(n / (med * 1e-3)),
              "time_over_kruskal_wallis": round(med / yard, 3)}, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--groups", type=int, default=100000)
    ap.add_argument("--rows", default="100,1000,5000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "categorical_test_bench.jsonl"))
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
    ctx.close()


if __name__ == "__main__":
    main()
