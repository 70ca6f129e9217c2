"""Grouped AFT fits next to OLS on the same device-resident rows: device-event time per call, the two calls alternated in one
process (OLS of log t, then the Weibull AFT fit with about 30 % of the rows censored, both with an intercept), min / median / max
over the repetitions, the Newton iterations per fit, the time per iteration and the bytes a pass over the rows reads against the
time it takes.  One JSON line per shape, appended to profiles/aft_bench.jsonl with --out.

    python scripts/aft_bench.py [--reps 5] [--scale 1.0] [--shapes 100000x200x3,100000x200x8] [--dist weibull] [--predict] [--out FILE]

--predict alternates a third call, the fit-predict (quantile 0.5, horizon 1) into a preallocated [N, 4] tensor, and reports what the
prediction pass adds to the fit: in ms, as a ratio, and in units of one Newton iteration.

--scale multiplies the group counts (smaller runs of the same shapes).  The OLS time is context only: OLS is one pass over the
rows; a Newton iteration is one pass for l, g and -H plus one likelihood-only pass per trial step, the start adds two passes, the
intercept-only model its own iterations on log t and the event column alone."""
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


def make_data(G, n, p, dev, share=0.3):
    """Weibull times from the model itself; a censored row's time is the event time shortened by a uniform factor."""
    gen = torch.Generator(device=dev).manual_seed(1)
    N = G * n
    off = torch.arange(G + 1, dtype=torch.int64, device=dev) * n
    xs = [2.0 * torch.rand(N, dtype=torch.float64, device=dev, generator=gen) - 1.0 for _ in range(p)]
    beta = (torch.rand(p, dtype=torch.float64, device=dev, generator=gen) - 0.5) / p ** 0.5
    u = 0.01 + 0.98 * torch.rand(N, dtype=torch.float64, device=dev, generator=gen)
    logt = 1.0 + 0.8 * torch.log(-torch.log1p(-u))
    for j in range(p):
        logt += beta[j] * xs[j]
    cens = torch.rand(N, dtype=torch.float64, device=dev, generator=gen) < share
    shrink = 0.5 + 0.5 * torch.rand(N, dtype=torch.float64, device=dev, generator=gen)
    time = torch.exp(logt) * torch.where(cens, shrink, torch.ones_like(shrink))
    event = (~cens).to(torch.float64)
    return off, xs, time, event


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--shapes", default="100000x200x3,100000x200x8")
    ap.add_argument("--dist", default="weibull")
    ap.add_argument("--predict", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    for shape in args.shapes.split(","):
        G, n, p = (int(v) for v in shape.split("x"))
        G = max(1, int(G * args.scale))
        off, xs, time, event = make_data(G, n, p, dev)
        logt = torch.log(time)
        ctx = pkg.Context(0)
        ols = pkg.RegressionOptions().batch_options("ols")
        aft = pkg.parse_aft_options({"dist": args.dist}).batch_options()
        times = {"ols": [], "aft": []}
        rec = None
        if args.predict:
            times["aft_predict"] = []
            predict = pkg.parse_aft_options({"quantile": 0.5, "horizon": 1.0}).predict_options()
            pred = torch.empty((G * n, 4), dtype=torch.float64, device=dev)
        for rep in range(args.reps + 1):  # the first round warms up
            for name in times:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if name == "ols":
                    ctx.fit_batch_device(off, logt, xs, None, ols)
                elif name == "aft":
                    rec = ctx.aft_fit_batch_device(off, time, xs, event, aft)
                else:
                    ctx.aft_fit_predict_batch_device(off, time, xs, event, aft, predict, pred_out=pred)
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    times[name].append(e0.elapsed_time(e1))
        r = rec.cpu().numpy()
        ok = r[:, p + 12] == 0
        it = r[ok, p + 10]
        out = {"shape": [G, n, p], "dist": args.dist, "reps": args.reps, "censored_share": round(float(1.0 - event.mean().item()), 3)}
        for name, t in times.items():
            out[name + "_ms"] = [round(float(min(t)), 3), round(float(np.median(t)), 3), round(float(max(t)), 3)]  # min, median, max
        med = float(np.median(times["aft"]))
        out["aft_fits_per_s"] = round(G / (med * 1e-3))
        out["aft_over_ols"] = round(med / float(np.median(times["ols"])), 2)
        out["status_nonzero"] = int((~ok).sum())
        out["iterations"] = {"mean": round(float(it.mean()), 2), "p50": int(np.percentile(it, 50)), "p99": int(np.percentile(it, 99)),
                             "max": int(it.max())}
        # a pass of the main model reads time-or-log t, the event and p columns of every row; a Newton iteration makes two of them
        # (the sums, and the likelihood of the full step) when no step is halved
        pass_bytes = G * n * (p + 2) * 8
        out["ms_per_iteration"] = round(med / float(it.mean()), 4)
        out["pass_gbytes"] = round(pass_bytes / 1e9, 3)
        out["tbytes_per_s_if_two_passes_per_iteration"] = round(2.0 * pass_bytes * float(it.mean()) / (med * 1e-3) / 1e12, 3)
        if args.predict:
            pmed = float(np.median(times["aft_predict"]))
            out["predict_pass_ms"] = round(pmed - med, 3)
            out["predict_over_fit"] = round(pmed / med, 4)
            out["predict_pass_in_iterations"] = round((pmed - med) / (med / float(it.mean())), 3)
            out["pred_gbytes_written"] = round(G * n * 32 / 1e9, 3)
        ctx.close()
        line = json.dumps(out)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        del xs, time, event, logt, rec
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
