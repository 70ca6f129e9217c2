"""Elastic net and NNLS end to end from page-locked host rows to records, two ways on the same rows:
  (a) state   rows in random slot order -> AggState.update (the streaming ingest) -> finalize_elasticnet / finalize_bls;
  (b) batch   the same rows pre-grouped, column-major -> elasticnet_fit_batch_host / bls_fit_batch_host (the path the DuckDB
              glue of the two families takes after buffering its rows; the grouping itself is NOT timed).
plus the time of a second elastic net Finalize with another lambda on the state of (a) (no row is touched again).  Creating
the state (allocation of its moment arrays, staging and, with --retain, the row log) is timed on its own ("create") and is NOT
part of leg (a): leg (b) runs on the context's workspace, which the warm-up round has grown already, and a query creates its
state once.  Wall-clock
times around synchronous calls, the legs alternated, one warm-up round, min / median / max over the repetitions.  Appends one
JSON line per shape to profiles/state_models_bench.jsonl.

    python scripts/state_models_bench.py [--reps 3] [--scale 1.0] [--shapes 1000000x100x3,100000x1000x8] [--retain]

--scale multiplies the group counts; --retain keeps a row log in HBM (exactly fitting slots are then refitted, not flagged)."""
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


def pinned(shape, dtype):
    return torch.empty(shape, dtype=dtype).pin_memory().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--shapes", default="1000000x100x3,100000x1000x8")
    ap.add_argument("--retain", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "state_models_bench.jsonl"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = pkg.Context(0)
    for shape in args.shapes.split(","):
        G, n, p = (int(v) for v in shape.split("x"))
        G = max(1, int(G * args.scale))
        N = G * n
        rng = np.random.default_rng(1)
        # grouped rows (b): column-major
        cols = [pinned((N,), torch.float64) for _ in range(p)]
        gy = pinned((N,), torch.float64)
        beta = rng.uniform(0.5, 2.0, p)
        gy[:] = 1.0 + 0.5 * rng.standard_normal(N)
        for j in range(p):
            cols[j][:] = rng.standard_normal(N)
            gy += beta[j] * cols[j]
        offs = np.arange(G + 1, dtype=np.int64) * n
        # the same rows in arrival order (a): row-major, slots shuffled
        perm = rng.permutation(N)
        slot = pinned((N,), torch.int32).view(np.uint32)
        slot[:] = (perm // n).astype(np.uint32)
        y = pinned((N,), torch.float64)
        y[:] = gy[perm]
        X = pinned((N, p), torch.float64)
        for j in range(p):
            X[:, j] = cols[j][perm]
        del perm
        en = [pkg.ElasticNetOptions(alpha=a, l1_ratio=0.5).batch_options() for a in (0.1 * n, 0.3 * n)]
        nnls = pkg.BlsOptions(fit_intercept=True).batch_options()
        ols = pkg.RegressionOptions(fit_intercept=True).batch_options("ols")
        t = {k: [] for k in ("en_state", "en_batch", "nnls_state", "nnls_batch", "en_second_finalize", "ingest", "create")}
        unref = {}
        for rep in range(args.reps + 1):                 # the first round warms up
            for fam in ("en", "nnls"):
                tc = time.perf_counter()
                st = pkg.AggState(ctx, p, ols, initial_slots=G, retain_bytes=(64 << 30) if args.retain else 0)
                ctx.synchronize()
                t0 = time.perf_counter()
                st.update(slot, y, X, n_slots=G)
                ctx.synchronize()
                t1 = time.perf_counter()
                rec, its, un = st.finalize_elasticnet(en[0]) if fam == "en" else st.finalize_bls(nnls)
                t2 = time.perf_counter()
                if fam == "en":
                    st.finalize_elasticnet(en[1])
                    t3 = time.perf_counter()
                st.close()
                tb0 = time.perf_counter()
                if fam == "en":
                    brec, _ = pkg.elasticnet_fit_batch_host(offs, gy, cols, en[0], ctx=ctx)
                else:
                    brec, _ = pkg.bls_fit_batch_host(offs, gy, cols, nnls, ctx=ctx)
                tb1 = time.perf_counter()
                unref[fam] = int(len(un))
                if rep:
                    t[fam + "_state"].append(1e3 * (t2 - t0))
                    t[fam + "_batch"].append(1e3 * (tb1 - tb0))
                    if fam == "en":
                        t["ingest"].append(1e3 * (t1 - t0))
                        t["create"].append(1e3 * (t0 - tc))
                        t["en_second_finalize"].append(1e3 * (t3 - t2))
                else:
                    ok = rec[:, p + 5] == 0
                    err = float(np.nanmax(np.abs(rec[ok, :p] - brec[ok, :p]))) if ok.any() else 0.0
                    unref[fam + "_max_abs_coef_diff"] = err
        out = {"shape": [G, n, p], "reps": args.reps, "retain": bool(args.retain), "unrefined": unref}
        for k, v in t.items():
            out[k + "_ms"] = [round(float(min(v)), 2), round(float(np.median(v)), 2), round(float(max(v)), 2)]
        for fam in ("en", "nnls"):
            out[fam + "_state_over_batch"] = round(float(np.median(t[fam + "_state"]) / np.median(t[fam + "_batch"])), 3)
        line = json.dumps(out)
        print(line, flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        del cols, gy, slot, y, X
    ctx.close()


if __name__ == "__main__":
    main()
