"""Grouped bounded least squares against ridge on the same device-resident data: device-event time per call, the calls
alternated in one process (ridge, NNLS without an intercept, a two-sided box with an intercept), ranges over the repetitions,
plus the outer iterations per group (mean, max).  One JSON line per shape.

    python scripts/bls_bench.py [--reps 5] [--scale 1.0] [--shapes 1000000x1000x8,100000x1000x32,50000x1000x64,20000x4096x128]

--scale multiplies the group counts (smaller runs of the same shapes)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--shapes", default="1000000x1000x8,100000x1000x32,50000x1000x64,20000x4096x128")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    for shape in args.shapes.split(","):
        G, n, p = (int(v) for v in shape.split("x"))
        G = max(1, int(G * args.scale))
        gen = torch.Generator(device=dev).manual_seed(1)
        off = torch.arange(G + 1, dtype=torch.int64, device=dev) * n
        xs = [torch.randn(G * n, dtype=torch.float64, device=dev, generator=gen) for _ in range(p)]
        beta = torch.randn(p, dtype=torch.float64, device=dev, generator=gen)
        y = 0.5 * torch.randn(G * n, dtype=torch.float64, device=dev, generator=gen) + 1.0
        for j in range(p):
            y += beta[j] * xs[j]
        ctx = pkg.Context(0)
        ridge = pkg.RegressionOptions(alpha=1.0).batch_options("ridge")
        legs = {"nnls": pkg.BlsOptions(), "box": pkg.BlsOptions(fit_intercept=True, lower_bound=-0.5, upper_bound=0.5)}
        opts = {k: v.batch_options() for k, v in legs.items()}
        core = torch.empty((G, p + 6), dtype=torch.float64, device=dev)
        rec = torch.empty((G, 3 * p + 6), dtype=torch.float64, device=dev)
        its = {k: torch.empty((G,), dtype=torch.int32, device=dev) for k in legs}
        times = {"ridge": [], "nnls": [], "box": []}
        for rep in range(args.reps + 1):  # the first round warms up
            for name in times:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if name == "ridge":
                    ctx.fit_batch_device(off, y, xs, None, ridge, core=core)
                else:
                    ctx.bls_fit_batch_device(off, y, xs, opts[name], records=rec, iterations=its[name])
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    times[name].append(e0.elapsed_time(e1))
        out = {"shape": [G, n, p], "reps": args.reps}
        for name, t in times.items():
            out[name + "_ms"] = [round(float(min(t)), 3), round(float(np.median(t)), 3), round(float(max(t)), 3)]  # min, median, max
        for name in legs:
            it = np.abs(its[name].cpu().numpy())
            out[name + "_ratio"] = round(float(np.median(times[name]) / np.median(times["ridge"])), 3)
            out[name + "_iterations_mean"] = round(float(it.mean()), 2)
            out[name + "_iterations_max"] = int(it.max())
            out[name + "_hit_limit"] = int((its[name].cpu().numpy() < 0).sum())
        ctx.close()
        print(json.dumps(out), flush=True)
        del xs, y, core, rec, its
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
