"""Elastic net fit-predict against ridge on the same device-resident data, at the reference's published window shape
(1M partitions x 100 rows x 3 features, default options): the expanding window, a ROWS 20 PRECEDING window and the
fit-predict aggregate at 20 % prediction rows.  Device-event time per call (median of --reps after a warm-up), the frames
the window kernels flagged for a refit, and the sweeps (min / median / max): per group of the aggregate's fit, and per frame
for the window cases (the frames of the first 2000 partitions fitted as groups), with the median over wavefronts of each
wavefront's slowest frame.  One JSON line per case.

    python scripts/elasticnet_family_bench.py [--reps 3] [--scale 1.0] [--cases expanding,rolling20,agg]

Run it once as is and once with ANOFOX_EN_WINDOW_NARROW=0 (a separate process: the switch is read once) for the frames
path of the window cases."""
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


def _time(fn, reps):
    out = []
    for rep in range(reps + 1):  # the first call warms up
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if rep:
            out.append(e0.elapsed_time(e1))
    return float(np.median(out))


def _sweeps(ctx, en, y, xs, n, frame, sample):
    """Sweeps per frame (min / median / max) and per wavefront of 8-lane segments (max over each 64 consecutive frames:
    what a wave of the in-register kernels waits for), from the batch fit of the first `sample` partitions' frames
    materialised as groups."""
    dev = y.device
    e = torch.arange(sample * n, device=dev)
    start = (e // n) * n
    lo = start if frame[0] is None else torch.maximum(start, e - frame[0])
    hi = e + 1
    lens = hi - lo
    off = torch.zeros(len(e) + 1, dtype=torch.int64, device=dev)
    off[1:] = torch.cumsum(lens, 0)
    idx = torch.repeat_interleave(lo, lens) + (torch.arange(int(off[-1]), device=dev) - torch.repeat_interleave(off[:-1], lens))
    core = torch.empty((len(e), len(xs) + 6), dtype=torch.float64, device=dev)
    its = torch.empty((len(e),), dtype=torch.int32, device=dev)
    ctx.elasticnet_fit_batch_device(off, y[idx].contiguous(), [x[idx].contiguous() for x in xs], en, core=core, iterations=its)
    torch.cuda.synchronize()
    it = np.abs(its.cpu().numpy())
    ok = core[:, len(xs) + 5].cpu().numpy() == 0
    # an output row's frame ends at that row; frames with too few rows are NULL in the window and not counted
    sw = it[ok]
    per_wave = np.array([it[k:k + 64][ok[k:k + 64]].max(initial=0) for k in range(0, len(it), 64)])
    return {"sweeps_min": int(sw.min()), "sweeps_median": float(np.median(sw)), "sweeps_max": int(sw.max()),
            "wave_sweeps_median": float(np.median(per_wave))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--shape", default="1000000x100x3")
    ap.add_argument("--cases", default="expanding,rolling20,agg")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    G, n, p = (int(v) for v in args.shape.split("x"))
    G = max(1, int(G * args.scale))
    gen = torch.Generator(device=dev).manual_seed(1)
    off = torch.arange(G + 1, dtype=torch.int64, device=dev) * n
    xs = [torch.randn(G * n, dtype=torch.float64, device=dev, generator=gen) for _ in range(p)]
    beta = torch.randn(p, dtype=torch.float64, device=dev, generator=gen)
    y = 0.5 * torch.randn(G * n, dtype=torch.float64, device=dev, generator=gen) + 1.0
    for j in range(p):
        y += beta[j] * xs[j]
    ctx = pkg.Context(0)
    en = pkg.ElasticNetOptions().batch_options()          # the reference's defaults: alpha 1, l1_ratio 0.5
    ridge = pkg.RegressionOptions(alpha=1.0).batch_options("ridge")
    path = "frames" if os.environ.get("ANOFOX_EN_WINDOW_NARROW") == "0" else "narrow"
    pred = torch.empty((G * n, 3), dtype=torch.float64, device=dev)
    core = torch.empty((G, p + 6), dtype=torch.float64, device=dev)
    for case in args.cases.split(","):
        rec = {"case": case, "shape": [G, n, p], "en_path": path}
        if case in ("expanding", "rolling20"):
            frame = (None, 0) if case == "expanding" else (20, 0)
            rec["elasticnet_ms"] = round(_time(lambda: ctx.elasticnet_fit_predict_window_device(off, y, xs, en, frame, pred=pred), args.reps), 3)
            rec["flagged_frames"] = ctx.last_window_refit_count()
            rec["ridge_ms"] = round(_time(lambda: ctx.fit_predict_window_device(off, y, xs, None, ridge, frame, pred=pred), args.reps), 3)
            rec.update(_sweeps(ctx, en, y, xs, n, frame, min(G, 2000)))
        elif case == "agg":
            # 20 % prediction rows: their y is NULL (NaN), every row is predicted
            mask = torch.rand(G * n, generator=gen, device=dev, dtype=torch.float64) < 0.2
            y_fit = torch.where(mask, torch.full_like(y, float("nan")), y)
            rec["elasticnet_ms"] = round(_time(lambda: ctx.elasticnet_fit_predict_batch_device(off, y_fit, xs, en, core=core, pred=pred),
                                               args.reps), 3)
            rec["ridge_ms"] = round(_time(lambda: ctx.fit_predict_batch_device(off, y_fit, xs, None, ridge, core=core, pred=pred),
                                          args.reps), 3)
            its = torch.empty((G,), dtype=torch.int32, device=dev)
            ctx.elasticnet_fit_batch_device(off, y_fit, xs, en, core=core, iterations=its)
            torch.cuda.synchronize()
            it = its.cpu().numpy()
            sw = np.abs(it[core[:, p + 5].cpu().numpy() == 0])
            rec.update({"sweeps_min": int(sw.min()), "sweeps_median": float(np.median(sw)), "sweeps_max": int(sw.max()),
                        "hit_limit": int((it < 0).sum())})
            del y_fit, mask
        rec["ratio"] = round(rec["elasticnet_ms"] / rec["ridge_ms"], 3)
        print(json.dumps(rec), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
