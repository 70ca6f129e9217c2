"""The GLM window function against the only route there was before it: every frame's rows gathered into a group of its own on
the host and fitted by anofox_hip_glm_fit_predict_batch_host (the gather included in its time).  Host-resident Poisson data,
host entry points (the planner's host work and the staging are inside every figure), device events around each call after one
warm-up, wall time beside them.  Per shape one JSON line (appended to --out) with three legs: the walk with the warm start
(the default), the walk with every frame cold (the test hook), the gathered batch; and the stats record of both walks.

    python scripts/glm_window_bench.py [--reps 3] [--scale 1.0] [--shapes 10000x200x3:30,10000x200x3:u] [--chunk 500] [--out FILE]

A shape is partitions x rows x p : frame, the frame `N` = N PRECEDING .. CURRENT ROW or `u` = UNBOUNDED PRECEDING .. CURRENT ROW.
The gathered leg runs once, in chunks of --chunk partitions (the gathered rows of the unbounded shape would not fit in one
staging buffer comfortably); its time is the sum over the chunks.  No ratio is asserted."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("anofox-statistics_amd")


def make_data(G, n, p):
    rng = np.random.default_rng(1)
    x = rng.uniform(-1.0, 1.0, size=(G * n, p))
    b = rng.normal(size=(G, p))
    b *= rng.uniform(0.3, 2.2, size=(G, 1)) / np.abs(b).sum(axis=1, keepdims=True)
    eta = np.einsum("gnp,gp->gn", x.reshape(G, n, p), b).ravel() + 1.0
    y = rng.poisson(np.exp(eta)).astype(np.float64)
    return np.arange(G + 1, dtype=np.int64) * n, y, [np.ascontiguousarray(x[:, j]) for j in range(p)]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), 1e3 * (time.perf_counter() - t0), out


def spread(t):
    return [round(float(min(t)), 3), round(float(np.median(t)), 3), round(float(max(t)), 3)]


def gathered(off, y, cols, start, opts, g0, g1, n):
    """The frames of partitions [g0, g1) as groups of a batch call: the gather on the host, then the fit."""
    r = np.arange(g0 * n, g1 * n, dtype=np.int64)
    plo = (r // n) * n
    lo = plo if start is None else np.maximum(r - start, plo)
    lens = r + 1 - lo
    goff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = np.arange(goff[-1], dtype=np.int64) - np.repeat(goff[:-1] - lo, lens)
    core, pred = pkg.glm_fit_predict_batch_host(goff, y[idx], [c[idx] for c in cols], opts)
    return core, pred[goff[1:] - 1], int(goff[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--shapes", default="10000x200x3:30,10000x200x3:u")
    ap.add_argument("--chunk", type=int, default=500)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    opts = pkg.parse_poisson_options(None).batch_options()
    for shape in args.shapes.split(","):
        dims, frame = shape.split(":")
        G, n, p = (int(v) for v in dims.split("x"))
        G = max(1, int(G * args.scale))
        start = None if frame == "u" else int(frame)
        N = G * n
        off, y, cols = make_data(G, n, p)
        out = {"shape": [G, n, p], "frame": frame, "reps": args.reps, "output_rows": N}
        walks = {}
        for name, warm in (("warm", True), ("cold", False)):
            pkg.glm_window_test_hooks(0, 0, warm)
            ev, wall = [], []
            for rep in range(args.reps + 1):  # the first round warms up
                e, w, res = timed(lambda: pkg.glm_fit_predict_window_host(off, y, cols, opts, (start, 0), want_records=True))
                if rep:
                    ev.append(e)
                    wall.append(w)
            st = pkg.glm_window_stats()
            walks[name] = res
            ok = int((res[1][:, p + 10] == 0).sum())
            out.update({name + "_event_ms": spread(ev), name + "_wall_ms": spread(wall),
                        name + "_ns_per_row": round(1e6 * float(np.median(wall)) / N, 2), name + "_fitted_frames": ok,
                        name + "_iterations_per_frame": round(st["iterations"] / max(ok, 1), 3), name + "_stats": st})
        pkg.glm_window_test_hooks(0, 0, True)
        out["status_differs_warm_vs_cold"] = int((walks["warm"][1][:, p + 10] != walks["cold"][1][:, p + 10]).sum())
        if not args.no_baseline:
            gathered(off, y, cols, start, opts, 0, min(G, 8), n)  # warm-up
            ev = wall = rows = 0
            differs = 0
            for g0 in range(0, G, args.chunk):
                g1 = min(G, g0 + args.chunk)
                e, w, (core, pred, m) = timed(lambda: gathered(off, y, cols, start, opts, g0, g1, n))
                ev, wall, rows = ev + e, wall + w, rows + m
                differs += int(np.sum(core.tobytes() != walks["cold"][1][g0 * n:g1 * n].tobytes()))
            out.update({"gathered_event_ms": round(ev, 3), "gathered_wall_ms": round(wall, 3), "gathered_rows": rows,
                        "gathered_ns_per_row": round(1e6 * wall / N, 2), "gathered_chunks_differing_from_cold_walk": differs})
        line = json.dumps(out)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
