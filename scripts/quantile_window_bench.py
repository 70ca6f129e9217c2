"""The quantile regression window function against what a user had before it: the same frames materialised as groups (each
frame's rows copied out) and fitted cold with quantile_fit_batch_device.  Device-resident Gaussian data, device-event time,
the legs alternated in one process, one warm-up round, min / median / max over the repetitions.  Per shape one JSON line
(appended to --out): time per output row of the walk, of the cold fits and of the copy that materialises the frames (timed
on its own), mean pivots per frame of both, the share of fitted frames that restarted after a fitted frame because a basis row
left (and, separately, all frames begun afresh: each run's first fit and the frames after a failed one too), walkers,
launched wavefronts and scratch rows, and the largest relative difference between a walk loss and its cold loss with the output
row it occurs at and both losses.

    python scripts/quantile_window_bench.py [--reps 5] [--scale 1.0] [--shapes 100000x100x3:30,16x200000x3:100,100000x100x8:u] [--out FILE]

A shape is partitions x rows x p : frame, the frame `N` = N PRECEDING .. CURRENT ROW or `u` = UNBOUNDED PRECEDING .. CURRENT ROW;
tau = 0.5 with an intercept.  --scale multiplies the partition counts (smaller runs of the same shapes).  --no-baseline skips the
cold leg."""
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


def make_data(G, n, p, dev):
    gen = torch.Generator(device=dev).manual_seed(1)
    off = torch.arange(G + 1, dtype=torch.int64, device=dev) * n
    xs = [torch.randn(G * n, dtype=torch.float64, device=dev, generator=gen) for _ in range(p)]
    beta = torch.randn(p, dtype=torch.float64, device=dev, generator=gen)
    y = 0.5 * torch.randn(G * n, dtype=torch.float64, device=dev, generator=gen) + 1.0
    for j in range(p):
        y += beta[j] * xs[j]
    return off, xs, y


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def stats(t):
    return [round(float(min(t)), 3), round(float(np.median(t)), 3), round(float(max(t)), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--shapes", default="100000x100x3:30,16x200000x3:100,100000x100x8:u")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    for shape in args.shapes.split(","):
        dims, frame = shape.split(":")
        G, n, p = (int(v) for v in dims.split("x"))
        G = max(1, int(G * args.scale))
        start = None if frame == "u" else int(frame)
        N = G * n
        off, xs, y = make_data(G, n, p, dev)
        ctx = pkg.Context(0)
        o = pkg.QuantileOptions(tau=0.5).batch_options()
        # the frames as the ROWS entry point clips them, and as groups of a batch call
        r = torch.arange(N, dtype=torch.int64, device=dev)
        plo = (r // n) * n
        lo = plo if start is None else torch.maximum(r - start, plo)
        hi = r + 1
        t_walk, t_copy, t_cold = [], [], []
        walk = cold = None
        for rep in range(args.reps + 1):  # the first round warms up
            ms, walk = timed(lambda: ctx.quantile_fit_predict_window_device(off, y, xs, o, (start, 0), want_records=True))
            if rep:
                t_walk.append(ms)
            if rep == 0:
                st = ctx.quantile_window_stats()
            if args.no_baseline:
                continue

            def materialise():
                lens = hi - lo
                goff = torch.zeros(N + 1, dtype=torch.int64, device=dev)
                torch.cumsum(lens, 0, out=goff[1:])
                total = int(goff[-1].item())
                idx = torch.arange(total, dtype=torch.int64, device=dev) - torch.repeat_interleave(goff[:-1] - lo, lens, output_size=total)
                return goff, y[idx], [c[idx] for c in xs]

            ms, (goff, yg, xg) = timed(materialise)
            if rep:
                t_copy.append(ms)
            ms, cold = timed(lambda: ctx.quantile_fit_batch_device(goff, yg, xg, o))
            if rep:
                t_cold.append(ms)
            rows_materialised = int(yg.numel())
            del goff, yg, xg
        pred, rec, its = walk
        ok = rec[:, p + 5] == 0
        out = {"shape": [G, n, p], "frame": frame, "reps": args.reps, "output_rows": N, "fitted_frames": int(ok.sum().item()),
               "walk_ms": stats(t_walk), "walk_ns_per_row": round(1e6 * float(np.median(t_walk)) / N, 2),
               "walk_pivots_per_frame": round(float(its[ok].abs().double().mean().item()), 3),
               "walk_hit_limit": int((its < 0).sum().item()),
               # restarts: frames begun afresh right after a fitted frame (on ROWS frames: a basis row left) — the share that phantom
               # basis elements would remove; begun_afresh also counts each run's first fit and the frames after a failed one
               "restart_share": round(st["restarts"] / max(int(ok.sum().item()), 1), 4), "restarts": st["restarts"],
               "begun_afresh_share": round(st["cold_starts"] / max(int(ok.sum().item()), 1), 4), "begun_afresh": st["cold_starts"],
               "walkers": st["walkers"], "waves": st["waves"], "span_rows": st["span_rows"]}
        if not args.no_baseline:
            crec, cits = cold
            # |walk - cold| / max(cold, 1e-9) over the fitted frames; the worst frame's output row and both of its losses go into the line
            rel = torch.where(ok, (rec[:, p + 2] - crec[:, p + 2]).abs() / crec[:, p + 2].abs().clamp_min(1e-9), torch.zeros_like(rec[:, 0]))
            worst = int(rel.argmax().item())
            out.update({"copy_ms": stats(t_copy), "cold_ms": stats(t_cold), "rows_materialised": rows_materialised,
                        "copy_ns_per_row": round(1e6 * float(np.median(t_copy)) / N, 2),
                        "cold_ns_per_row": round(1e6 * float(np.median(t_cold)) / N, 2),
                        "cold_pivots_per_frame": round(float(cits[ok].abs().double().mean().item()), 3),
                        "cold_hit_limit": int((cits < 0).sum().item()),
                        "walk_over_cold": round(float(np.median(t_walk) / np.median(t_cold)), 3),
                        "walk_over_cold_plus_copy": round(float(np.median(t_walk) / (np.median(t_cold) + np.median(t_copy))), 3),
                        "status_differs": int((rec[:, p + 5] != crec[:, p + 5]).sum().item()),
                        "max_rel_loss_diff": float(rel[worst].item()), "worst_frame": worst,
                        "worst_frame_losses": [float(rec[worst, p + 2].item()), float(crec[worst, p + 2].item())]})
        ctx.close()
        line = json.dumps(out)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        del xs, y, walk, cold, pred, rec, its
        rel = crec = cits = None
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
