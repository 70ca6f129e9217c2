"""Recursive least squares against ridge on the same device-resident data.  Legs (each with ridge's time on the same shape):
  batch      G groups x n rows x p features (--batch 1000000x1000x8,...; the issue's shapes are 1M x 1000 x {8, 32, 64})
  expanding  the reference's window shape, P partitions x n rows x 3, frame {UNBOUNDED PRECEDING, CURRENT ROW}
  rolling20  the same with ROWS 19 PRECEDING
  long       one group of R rows at p = 8 (the long-group route)
Device-event time per call (median of --reps after a warm-up).  One JSON line per leg, appended to profiles/rls_bench.jsonl.

    python scripts/rls_bench.py [--reps 3] [--batch 100000x1000x8] [--window 1000000x100] [--long 50000000] [--legs batch,expanding,rolling20,long]

Run once more with ANOFOX_RLS_EXPANDING=0 (a separate process: the switch is read once) for the frames path of the expanding leg,
and with ANOFOX_RLS_LONG_ROWS=<rows> to move the long-group threshold."""
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


def _data(G, n, p, dev):
    gen = torch.Generator(device=dev).manual_seed(1)
    N = G * n
    X = torch.randn((p, N), generator=gen, device=dev, dtype=torch.float64)
    y = X.sum(0) * 0.5 + 0.1 * torch.randn(N, generator=gen, device=dev, dtype=torch.float64)
    off = torch.arange(0, N + 1, n, device=dev, dtype=torch.int64)
    return off, y, [X[j].contiguous() for j in range(p)]


def _shape(s):
    return [int(v) for v in s.split("x")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", default="100000x1000x8,100000x1000x32,20000x1000x64")
    ap.add_argument("--window", default="1000000x100")
    ap.add_argument("--long", type=int, default=50_000_000)
    ap.add_argument("--legs", default="batch,expanding,rolling20,long")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rls_bench.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = pkg.Context()
    rls = pkg.RlsOptions().batch_options()
    ridge = pkg.RegressionOptions(alpha=1.0).batch_options("ridge")
    lines = []
    legs = a.legs.split(",")
    if "batch" in legs:
        for s in a.batch.split(","):
            G, n, p = _shape(s)
            off, y, xs = _data(G, n, p, dev)
            t = _time(lambda: ctx.rls_fit_batch_device(off, y, xs, rls), a.reps)
            tr = _time(lambda: ctx.fit_batch_device(off, y, xs, None, ridge), a.reps)
            lines.append({"leg": "batch", "groups": G, "rows": n, "p": p, "rls_ms": t, "ridge_ms": tr, "ratio": t / tr})
            del off, y, xs
    if "expanding" in legs or "rolling20" in legs:
        P, n = _shape(a.window)
        off, y, xs = _data(P, n, 3, dev)
        for leg, frame in (("expanding", (None, 0)), ("rolling20", (19, 0))):
            if leg not in legs:
                continue
            t = _time(lambda: ctx.rls_fit_predict_window_device(off, y, xs, rls, frame), a.reps)
            tr = _time(lambda: ctx.fit_predict_window_device(off, y, xs, None, ridge, frame=frame), a.reps)
            lines.append({"leg": leg, "partitions": P, "rows": n, "p": 3, "rls_ms": t, "ridge_ms": tr, "ratio": t / tr,
                          "expanding_kernel": os.environ.get("ANOFOX_RLS_EXPANDING", "1") != "0"})
        del off, y, xs
    if "long" in legs:
        off, y, xs = _data(1, a.long, 8, dev)
        t = _time(lambda: ctx.rls_fit_batch_device(off, y, xs, rls), max(1, a.reps // 3))
        tr = _time(lambda: ctx.fit_batch_device(off, y, xs, None, ridge), a.reps)
        lines.append({"leg": "long", "groups": 1, "rows": a.long, "p": 8, "rls_ms": t, "ridge_ms": tr, "ratio": t / tr,
                      "long_rows": int(os.environ.get("ANOFOX_RLS_LONG_ROWS", 1 << 16))})
    with open(a.out, "a") as f:
        for ln in lines:
            print(json.dumps(ln), flush=True)
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
