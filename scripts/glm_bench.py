"""Stand-alone timing of the fused GLM kernel against the only alternative that needs no new kernel: the WLS batch path
(Context.fit_batch_device with per-row weights w and working response z) called once per IRLS iteration from the host, with an
elementwise torch step between the calls, run to the fused kernel's iteration count.

    python scripts/glm_bench.py [--shapes 10000x1000x3,10000x1000x8,10000x1000x32,1000000x100x3] [--reps 5] [--inner 10] [--out FILE]

Both paths are warmed up once per shape and timed alternately (fused, host loop, fused, ...).  A timed window is `inner` calls
enqueued back to back and one device synchronise, under a host clock, so that a window lasts tens of milliseconds at the
least; the per-call median and range over `reps` windows are reported.  The traffic figure is computed from the
shapes: per iteration the fused kernel reads the p columns twice (the Gram pass and the eta pass), y twice, and reads and writes the
2 doubles of scratch per row; the first, the finishing and the inference passes add about three more sweeps.  Whether those
bytes come from HBM or from L2 is not measured here."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "anofox-statistics_amd"


def make(G, n, p, family, device, seed=3):
    import torch
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    N = G * n
    x = [torch.rand(N, generator=g, device=device, dtype=torch.float64) * 2 - 1 for _ in range(p)]
    b = torch.randn(G, p, generator=g, device=device, dtype=torch.float64)
    b = b * (1.5 / b.abs().sum(1, keepdim=True))
    eta = torch.zeros(N, device=device, dtype=torch.float64)
    for j in range(p):
        eta += x[j] * b[:, j].repeat_interleave(n)
    if family == 0:
        y = torch.poisson(torch.exp(eta + 1.0), generator=g)
    else:
        y = (torch.rand(N, generator=g, device=device, dtype=torch.float64) < torch.sigmoid(eta)).double()
    offs = torch.arange(0, N + 1, n, device=device, dtype=torch.int64)
    return offs, y, x


def host_loop(pkg, ctx, offs, y, x, family, n, iters):
    """IRLS through the WLS batch path: one fit_batch_device call per iteration, an elementwise torch step between them."""
    import torch
    p = len(x)
    opts = pkg.RegressionOptions(compute_inference=False).batch_options("wls")
    mu = y + 0.1 if family == 0 else (y + 0.5) / 2
    eta = torch.log(mu) if family == 0 else torch.log(mu / (1 - mu))
    core = None
    for _ in range(iters):
        w = mu if family == 0 else mu * (1 - mu)
        z = eta + (y - mu) / w
        core, _ = ctx.fit_batch_device(offs, z, x, w, opts)
        eta = core[:, p].repeat_interleave(n)
        for j in range(p):
            eta = eta + x[j] * core[:, j].repeat_interleave(n)
        mu = torch.exp(eta) if family == 0 else torch.sigmoid(eta)
    return core


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="10000x1000x3,10000x1000x8,10000x1000x32,1000000x100x3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "glm_bench.py needs a GPU"
    pkg = importlib.import_module(PKG)
    abi = importlib.import_module(PKG + "._abi")
    ctx = pkg.Context(0)
    rows = []
    for shape in a.shapes.split(","):
        G, n, p = (int(v) for v in shape.split("x"))
        for family, name in ((0, "poisson"), (1, "logistic")):
            offs, y, x = make(G, n, p, family, "cuda:0")
            opts = abi.AnofoxHipGlmBatchOptions(family, True, 100, 1e-8, 0.0, False, 0.95)

            def fused():
                rec = ctx.glm_fit_batch_device(offs, y, x, opts)
                torch.cuda.synchronize()
                return rec
            rec = fused()                                             # warm-up, and the iteration counts
            st = rec[:, p + 10]
            its = rec[:, p + 8][st == 0]
            iters = int(its.max().item())
            core = host_loop(pkg, ctx, offs, y, x, family, n, iters)  # warm-up
            torch.cuda.synchronize()
            ok = st == 0
            err = float((core[ok][:, :p + 1] - rec[ok][:, :p + 1]).abs().max().item())
            tf, th = [], []
            for _ in range(a.reps):                                   # each window: `inner` calls, then one synchronise
                t0 = time.perf_counter()
                for _ in range(a.inner):
                    ctx.glm_fit_batch_device(offs, y, x, opts)
                torch.cuda.synchronize()
                tf.append((time.perf_counter() - t0) / a.inner)
                t0 = time.perf_counter()
                for _ in range(a.inner):
                    host_loop(pkg, ctx, offs, y, x, family, n, iters)
                torch.cuda.synchronize()
                th.append((time.perf_counter() - t0) / a.inner)
            N = G * n
            mean_it = float(its.mean().item())
            bytes_est = 8.0 * N * ((2 * (p + 1) + 4) * mean_it + 3 * (p + 1))
            row = dict(shape=shape, family=name, groups_ok=int(ok.sum().item()), iterations_max=iters, iterations_mean=round(mean_it, 2),
                       fused_ms_median=1e3 * float(np.median(tf)), fused_ms_min=1e3 * min(tf), fused_ms_max=1e3 * max(tf),
                       host_loop_ms_median=1e3 * float(np.median(th)), host_loop_ms_min=1e3 * min(th), host_loop_ms_max=1e3 * max(th),
                       traffic_gb_estimate=bytes_est / 1e9, fused_gb_per_s_estimate=bytes_est / 1e9 / float(np.median(tf)),
                       max_abs_coef_difference=err)
            print(json.dumps(row), flush=True)
            rows.append(row)
            del offs, y, x, rec, core
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
