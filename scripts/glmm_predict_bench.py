"""glmm fit-predict against the fit on device-resident arrays, on the shapes and with the timing method of scripts/glmm_bench.py:
device-event time per call (min / median / max over the repetitions, two warm-up calls), the time the prediction pass adds (the
difference of the medians) and the rate of the bytes that pass has to move once (8 p read and 40 written per row; the level and
panel records it also reads are small against them) beside the device's read rate (csrc/tools/hbm_read_rate, its best line).
One JSON line per shape, appended to profiles/glmm_predict_bench.jsonl with --out.

    python scripts/glmm_predict_bench.py [--reps 7] [--shapes 1x100000x15x3,1000x100x15x3,100000x4x5x1] [--out FILE]

A shape is panels x levels per panel x rows per level x p."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
pkg = importlib.import_module("anofox-statistics_amd")
from glmm_bench import hbm_read_rate, make_data   # noqa: E402


def time_call(fn, data, reps):
    times, out = [], None
    for r in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn(*data, {"interval": "prediction"})
        b.record()
        torch.cuda.synchronize()
        if r >= 2:   # (two warm-up calls)
            times.append(a.elapsed_time(b))
    return {"min": round(float(np.min(times)), 4), "median": round(float(np.median(times)), 4), "max": round(float(np.max(times)), 4)}, out


def measure(ctx, G, L, m, p, reps, dev, read_rate):
    data = make_data(G, L, m, p, dev)
    rows = G * L * m
    row = {"panels": G, "levels_per_panel": L, "rows_per_level": m, "p": p, "rows": rows, "predict_bytes": (8 * p + 40) * rows}
    pkg.glmm_test_hooks()
    row["fit_ms"], fit = time_call(ctx.glmm_fit_batch_device, data, reps)
    row["fit_predict_ms"], out = time_call(ctx.glmm_fit_predict_batch_device, data, reps)
    assert all(torch.equal(a, b) for a, b in zip(fit, out[:4]) if a is not None), "the fit's outputs differ"
    assert bool(torch.isfinite(out[4][:, :3]).all()), "a row was not scored"
    added = row["fit_predict_ms"]["median"] - row["fit_ms"]["median"]
    row["added_ms"] = round(added, 4)
    row["added_share"] = round(added / row["fit_ms"]["median"], 4)
    row["predict_gbps"] = round(row["predict_bytes"] / (added * 1e-3) / 1e9, 1) if added > 0 else None
    row["hbm_read_rate_gbps"] = read_rate
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
