"""Grouped quantile regression next to ridge on the same device-resident data: device-event time per call, the calls
alternated in one process (ridge, tau = 0.5, tau = 0.9, both with an intercept), min / median / max over the repetitions, plus
the distribution of simplex pivots per group.  One JSON line per shape, appended to profiles/quantile_bench.jsonl with --out.

    python scripts/quantile_bench.py [--reps 5] [--scale 1.0] [--shapes 100000x100x3,10000x1000x8] [--out FILE]

--scale multiplies the group counts (smaller runs of the same shapes).  The ridge time is context only: ridge is one pass
over the rows, the simplex makes several passes per pivot.

    python scripts/quantile_bench.py --path [--reps 5] [--scale 1.0] [--shapes ...] [--out FILE]

Path mode: the seven-tau path (0.05, 0.1, 0.25, 0.5, 0.75, 0.9, 0.95; one quantile_fit_path_batch_device call) against seven
single-tau device calls on the same resident inputs, alternated in one process, device-event time over each leg; min / median /
max over the repetitions, the ratio of the medians and the mean pivots per tau of both."""
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


PATH_TAUS = (0.05, 0.1, 0.25, 0.5, 0.75, 0.9, 0.95)


def make_data(G, n, p, dev):
    gen = torch.Generator(device=dev).manual_seed(1)
    off = torch.arange(G + 1, dtype=torch.int64, device=dev) * n
    xs = [torch.randn(G * n, dtype=torch.float64, device=dev, generator=gen) for _ in range(p)]
    beta = torch.randn(p, dtype=torch.float64, device=dev, generator=gen)
    y = 0.5 * torch.randn(G * n, dtype=torch.float64, device=dev, generator=gen) + 1.0
    for j in range(p):
        y += beta[j] * xs[j]
    return off, xs, y


def path_mode(args, dev):
    T = len(PATH_TAUS)
    for shape in args.shapes.split(","):
        G, n, p = (int(v) for v in shape.split("x"))
        G = max(1, int(G * args.scale))
        off, xs, y = make_data(G, n, p, dev)
        ctx = pkg.Context(0)
        base = pkg.QuantileOptions().batch_options()
        opts = [pkg.QuantileOptions(tau=t).batch_options() for t in PATH_TAUS]
        rec_p = torch.empty((G, T, p + 6), dtype=torch.float64, device=dev)
        its_p = torch.empty((G, T), dtype=torch.int32, device=dev)
        rec_c = [torch.empty((G, p + 6), dtype=torch.float64, device=dev) for _ in PATH_TAUS]
        its_c = [torch.empty((G,), dtype=torch.int32, device=dev) for _ in PATH_TAUS]
        times = {"path": [], "cold": []}
        for rep in range(args.reps + 1):  # the first round warms up
            for name in times:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if name == "path":
                    ctx.quantile_fit_path_batch_device(off, y, xs, base, PATH_TAUS, records=rec_p, iterations=its_p)
                else:
                    for t in range(T):
                        ctx.quantile_fit_batch_device(off, y, xs, opts[t], records=rec_c[t], iterations=its_c[t])
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    times[name].append(e0.elapsed_time(e1))
        out = {"mode": "path", "shape": [G, n, p], "taus": list(PATH_TAUS), "reps": args.reps}
        for name, t in times.items():
            out[name + "_ms"] = [round(float(min(t)), 3), round(float(np.median(t)), 3), round(float(max(t)), 3)]  # min, median, max
        out["path_over_cold"] = round(float(np.median(times["path"]) / np.median(times["cold"])), 3)
        ip = its_p.cpu().numpy()
        ic = np.stack([i.cpu().numpy() for i in its_c], axis=1)
        out["path_pivots_per_tau"] = [round(float(v), 2) for v in np.abs(ip).mean(axis=0)]
        out["cold_pivots_per_tau"] = [round(float(v), 2) for v in np.abs(ic).mean(axis=0)]
        out["path_mean_pivots_per_tau"] = round(float(np.abs(ip).mean()), 2)
        out["cold_mean_pivots_per_tau"] = round(float(np.abs(ic).mean()), 2)
        out["hit_limit"] = [int((ip < 0).sum()), int((ic < 0).sum())]
        out["status_nonzero"] = int((rec_p[:, :, p + 5] != 0).sum().item())
        loss_c = torch.stack([r[:, p + 2] for r in rec_c], dim=1)
        out["max_rel_loss_diff"] = float(((rec_p[:, :, p + 2] - loss_c).abs() / loss_c.abs().clamp_min(1e-300)).max().item())
        ctx.close()
        line = json.dumps(out)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        del xs, y, rec_p, its_p, rec_c, its_c
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--shapes", default="100000x100x3,10000x1000x8")
    ap.add_argument("--out", default=None)
    ap.add_argument("--path", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    if args.path:
        return path_mode(args, dev)
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
        legs = {"tau0.5": pkg.QuantileOptions(tau=0.5), "tau0.9": pkg.QuantileOptions(tau=0.9)}
        opts = {k: v.batch_options() for k, v in legs.items()}
        core = torch.empty((G, p + 6), dtype=torch.float64, device=dev)
        recs = {k: torch.empty((G, p + 6), dtype=torch.float64, device=dev) for k in legs}
        its = {k: torch.empty((G,), dtype=torch.int32, device=dev) for k in legs}
        times = {"ridge": [], "tau0.5": [], "tau0.9": []}
        for rep in range(args.reps + 1):  # the first round warms up
            for name in times:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if name == "ridge":
                    ctx.fit_batch_device(off, y, xs, None, ridge, core=core)
                else:
                    ctx.quantile_fit_batch_device(off, y, xs, opts[name], records=recs[name], iterations=its[name])
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    times[name].append(e0.elapsed_time(e1))
        out = {"shape": [G, n, p], "reps": args.reps}
        for name, t in times.items():
            out[name + "_ms"] = [round(float(min(t)), 3), round(float(np.median(t)), 3), round(float(max(t)), 3)]  # min, median, max
        for name in legs:
            raw = its[name].cpu().numpy()
            it = np.abs(raw)
            out[name + "_ratio"] = round(float(np.median(times[name]) / np.median(times["ridge"])), 3)
            out[name + "_pivots"] = {"mean": round(float(it.mean()), 2), "p50": int(np.percentile(it, 50)), "p90": int(np.percentile(it, 90)),
                                     "p99": int(np.percentile(it, 99)), "max": int(it.max())}
            out[name + "_hit_limit"] = int((raw < 0).sum())
            out[name + "_status_nonzero"] = int((recs[name][:, p + 5] != 0).sum().item())
        ctx.close()
        line = json.dumps(out)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        del xs, y, core, recs, its
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
