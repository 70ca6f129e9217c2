"""Grouped elastic net against ridge on the same device-resident data: device-event time per call, the two alternated
in one process, plus the sweeps per group (min / median / max).  One JSON line per shape.

    python scripts/elasticnet_bench.py [--reps 5] [--scale 1.0] [--shapes 1000000x1000x8,100000x200x32,20000x1000x64]

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
    ap.add_argument("--shapes", default="1000000x1000x8,100000x200x32,20000x1000x64")
    ap.add_argument("--alpha", type=float, default=1.0)
    ap.add_argument("--l1", type=float, default=0.5)
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
        ridge = pkg.RegressionOptions(alpha=args.alpha).batch_options("ridge")
        en = pkg.ElasticNetOptions(alpha=args.alpha, l1_ratio=args.l1).batch_options()
        core = torch.empty((G, p + 6), dtype=torch.float64, device=dev)
        its = torch.empty((G,), dtype=torch.int32, device=dev)
        times = {"ridge": [], "elasticnet": []}
        for rep in range(args.reps + 1):  # the first round warms up
            for name in ("ridge", "elasticnet"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if name == "ridge":
                    ctx.fit_batch_device(off, y, xs, None, ridge, core=core)
                else:
                    ctx.elasticnet_fit_batch_device(off, y, xs, en, core=core, iterations=its)
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    times[name].append(e0.elapsed_time(e1))
        it = its.cpu().numpy()
        sweeps = np.abs(it[core[:, p + 5].cpu().numpy() == 0])
        ctx.close()
        r, e = float(np.median(times["ridge"])), float(np.median(times["elasticnet"]))
        print(json.dumps({"shape": [G, n, p], "ridge_ms": round(r, 3), "elasticnet_ms": round(e, 3), "ratio": round(e / r, 3),
                          "sweeps_min": int(sweeps.min()), "sweeps_median": float(np.median(sweeps)),
                          "sweeps_max": int(sweeps.max()), "hit_limit": int((it < 0).sum())}), flush=True)
        del xs, y, core, its
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
