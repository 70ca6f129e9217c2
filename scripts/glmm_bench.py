"""glmm_fit on device-resident arrays: device-event time per call (min / median / max over the repetitions), the level-statistics
stage alone (through the test hook) with the bytes it has to read once (8 (p + 1) per row) against the device's read rate
(csrc/tools/hbm_read_rate, its best line), the share of the call that the profile search takes, the mean evaluations of the
search, and what the device form's search launches for the two other workgroup sizes cost (the call with only the size its
panels need).  One JSON line per shape, appended to profiles/glmm_bench.jsonl with --out.

    python scripts/glmm_bench.py [--reps 7] [--shapes 1x100000x15x3,1000x100x15x3,100000x4x5x1] [--out FILE]

A shape is panels x levels per panel x rows per level x p."""
import argparse
import importlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("anofox-statistics_amd")


def hbm_read_rate():
    """the best TB/s line of csrc/tools/hbm_read_rate, run as a process of its own before this one opens the device; None: not built"""
    exe = os.path.join(ROOT, "anofox-statistics_amd", "csrc", "tools", "hbm_read_rate")
    if not os.path.exists(exe):
        return None
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120).stdout
    rates = [float(m) for m in re.findall(r"([0-9.]+) TB/s", out)]
    return max(rates) * 1000.0 if rates else None


def make_data(G, L, m, p, dev):
    gen = torch.Generator(device=dev).manual_seed(1)
    n = G * L * m
    rnd = lambda k, f=torch.randn: f(k, dtype=torch.float64, device=dev, generator=gen)   # noqa: E731
    cols = [rnd(n) for _ in range(p)]
    b = rnd(G * L).repeat_interleave(m)
    y = 1.0 + 0.5 * sum(cols) + b + 0.7 * rnd(n)
    plo = torch.arange(G + 1, dtype=torch.int64, device=dev) * L
    lro = torch.arange(G * L + 1, dtype=torch.int64, device=dev) * m
    return plo, lro, y, cols


def time_call(ctx, data, reps):
    times, out = [], None
    for r in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = ctx.glmm_fit_batch_device(*data)
        b.record()
        torch.cuda.synchronize()
        if r >= 2:   # (two warm-up calls)
            times.append(a.elapsed_time(b))
    return {"min": round(float(np.min(times)), 4), "median": round(float(np.median(times)), 4), "max": round(float(np.max(times)), 4)}, out


def measure(ctx, G, L, m, p, reps, dev, read_rate):
    data = make_data(G, L, m, p, dev)
    row = {"panels": G, "levels_per_panel": L, "rows_per_level": m, "p": p, "rows": G * L * m, "bytes_read_once": 8 * (p + 1) * G * L * m}
    pkg.glmm_test_hooks()
    row["call_ms"], out = time_call(ctx, data, reps)
    rec = out[0].cpu().numpy()
    assert np.all(rec[:, p + 12] == 0), "a panel failed"
    row["mean_iterations"] = round(float(rec[:, p + 10].mean()), 2)
    row["converged_share"] = float(rec[:, p + 11].mean())
    pkg.glmm_test_hooks(1, 0)
    row["stats_ms"], _ = time_call(ctx, data, reps)
    row["stats_gbps"] = round(row["bytes_read_once"] / (row["stats_ms"]["median"] * 1e-3) / 1e9, 1)
    row["hbm_read_rate_gbps"] = read_rate
    row["search_share"] = round(1.0 - row["stats_ms"]["median"] / row["call_ms"]["median"], 3)
    waves = 1 if L <= 64 else (4 if L <= 1024 else 16)
    pkg.glmm_test_hooks(0, {1: 1, 4: 2, 16: 4}[waves])
    row["call_one_launch_ms"], _ = time_call(ctx, data, reps)
    row["search_waves"] = waves
    pkg.glmm_test_hooks()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="1x100000x15x3,1000x100x15x3,100000x4x5x1")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    read_rate = hbm_read_rate()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    ctx = pkg.Context(0)
    for shape in args.shapes.split(","):
        G, L, m, p = (int(v) for v in shape.split("x"))
        line = json.dumps(measure(ctx, G, L, m, p, args.reps, dev, read_rate))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
