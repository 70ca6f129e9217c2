"""The permutation test aggregates on device-resident arrays: device-event time per call, min / median / max over the repetitions.
One JSON line per measurement, appended to --out (default profiles/perm_test_bench.jsonl).

    python scripts/perm_test_bench.py [--reps 3] [--groups 10000] [--rows 200] [--perm 1000] [--large-groups 100]
                                      [--large-rows 100000] [--baseline-groups 20] [--restate tests/perm_test_restate.py] [--out FILE]

Reports groups per second and lane-steps per second (rows x permutations per group: one step is one row of one relabelling) of
--groups groups of --rows rows for the energy distance, the permutation t-test and MMD, then the energy distance of --large-groups
groups of --large-rows rows (the large path).  The baseline is the same call by the numpy restatement of the tests on the CPU,
timed on --baseline-groups groups (one group of the large shape) and scaled to the call."""
import argparse
import importlib
import importlib.util
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("anofox-statistics_amd")
TESTS = (("energy_distance", 0), ("permutation_t_test", 1), ("mmd", 2))
SEED = 2026


def time_call(fn, reps, warm=1):
    times = []
    for r in range(reps + warm):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if r >= warm:
            times.append(a.elapsed_time(b))
    return float(np.min(times)), float(np.median(times)), float(np.max(times))


def emit(row, out):
    line = json.dumps(row)
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")


def shape(ctx, restate, tests, groups, rows, perm, reps, base_groups, out):
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    n = groups * rows
    v = torch.randn(n, dtype=torch.float64, device=dev, generator=gen)
    s = torch.randint(0, 2, (n,), dtype=torch.int32, device=dev, generator=gen)
    off = torch.arange(groups + 1, dtype=torch.int64, device=dev) * rows
    hv, hs, hoff = v[:base_groups * rows].cpu().numpy(), s[:base_groups * rows].cpu().numpy(), off[:base_groups + 1].cpu().numpy()
    for name, test in tests:
        o = pkg.PermTestOptions(perm, SEED)
        lo, med, hi = time_call(lambda: ctx.perm_test_batch_device(off, v, s, test, o), reps)
        row = {"method": name, "groups": groups, "rows": rows, "permutations": perm,
               "ms": {"min": round(lo, 3), "median": round(med, 3), "max": round(hi, 3)},
               "groups_per_s": round(groups / (med * 1e-3), 1), "lane_steps_per_s": round(groups * rows * perm / (med * 1e-3))}
        if restate is not None and base_groups > 0:
            t0 = time.perf_counter()
            restate.reference(hoff, hv, hs, test, 0, perm, SEED)
            cpu_ms = (time.perf_counter() - t0) * 1e3 * groups / base_groups
            row.update(cpu_restatement_ms=round(cpu_ms, 1), cpu_over_gpu=round(cpu_ms / med, 1))
        emit(row, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--groups", type=int, default=10000)
    ap.add_argument("--rows", type=int, default=200)
    ap.add_argument("--perm", type=int, default=1000)
    ap.add_argument("--large-groups", type=int, default=100)
    ap.add_argument("--large-rows", type=int, default=100000)
    ap.add_argument("--baseline-groups", type=int, default=20)
    ap.add_argument("--restate", default=os.path.join(ROOT, "tests", "perm_test_restate.py"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "perm_test_bench.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    restate = None
    if args.restate and os.path.exists(args.restate):
        spec = importlib.util.spec_from_file_location("perm_test_restate", args.restate)
        restate = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(restate)
    torch.cuda.set_device(0)
    ctx = pkg.Context(0)
    shape(ctx, restate, TESTS, args.groups, args.rows, args.perm, args.reps, min(args.baseline_groups, args.groups), args.out)
    if args.large_groups > 0:
        shape(ctx, restate, TESTS[:1], args.large_groups, args.large_rows, args.perm, args.reps, 1 if args.baseline_groups else 0, args.out)
    ctx.close()


if __name__ == "__main__":
    main()
