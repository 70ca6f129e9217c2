"""eb_shrink on device-resident arrays: device-event time per call of both paths (forced through the test hooks) and of the
library's own choice, min / median / max over the repetitions, against the bytes a call moves (three reads of two doubles and one
write of three per pair: 72 bytes).  One JSON line per shape, appended to profiles/eb_shrink_bench.jsonl with --out.

    python scripts/eb_shrink_bench.py [--reps 7] [--shapes 1x100000x1,1x100000x8,1x100000x32,100000x8x1] [--crossover] [--out FILE]

A shape is n_sets x items per set x n_cols (tight strides).  --crossover sweeps one set of 2^k items at n_cols 1, 8 and 32 and
prints both paths' times side by side: the size from which the chunk path is faster is the library's kEbCrossoverPairs."""
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


def make_data(n_sets, m, n_cols, dev):
    gen = torch.Generator(device=dev).manual_seed(1)
    n = n_sets * m * n_cols
    se = 0.1 + 0.4 * torch.rand(n, dtype=torch.float64, device=dev, generator=gen)
    est = 0.5 + 0.3 * torch.randn(n, dtype=torch.float64, device=dev, generator=gen) + se * torch.randn(n, dtype=torch.float64, device=dev,
                                                                                                        generator=gen)
    return torch.arange(n_sets + 1, dtype=torch.int64, device=dev) * m, est, se


def time_call(ctx, off, est, se, n_cols, reps):
    times = []
    for r in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        pkg.eb_shrink_batch_device(ctx, off, est, se, n_cols)
        b.record()
        torch.cuda.synchronize()
        if r >= 2:   # (two warm-up calls)
            times.append(a.elapsed_time(b))
    return float(np.min(times)), float(np.median(times)), float(np.max(times))


def measure(ctx, n_sets, m, n_cols, reps, dev):
    off, est, se = make_data(n_sets, m, n_cols, dev)
    row = {"n_sets": n_sets, "items_per_set": m, "n_cols": n_cols, "bytes": 72 * n_sets * m * n_cols}
    for name, path in (("set_path", 1), ("chunk_path", 2), ("library", 0)):
        pkg.eb_shrink_test_hooks(path, 0, 0)
        lo, med, hi = time_call(ctx, off, est, se, n_cols, reps)
        row[name + "_ms"] = {"min": round(lo, 4), "median": round(med, 4), "max": round(hi, 4)}
        row[name + "_gbps"] = round(row["bytes"] / (med * 1e-3) / 1e9, 1)
    pkg.eb_shrink_test_hooks()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="1x100000x1,1x100000x8,1x100000x32,100000x8x1")
    ap.add_argument("--crossover", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    ctx = pkg.Context(0)
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",") if s]
    if args.crossover:
        shapes = [(1, 1 << k, c) for c in (1, 8, 32) for k in range(6, 15)]
    for n_sets, m, n_cols in shapes:
        row = measure(ctx, n_sets, m, n_cols, args.reps, dev)
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
