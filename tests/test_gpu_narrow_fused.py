"""The fused accumulate + solve kernel of the narrow path (p <= 8) against the separate solve kernel, bit for bit.

ANOFOX_NARROW_FUSED is read once per process, so each side runs in a child process of its own (this file is also the
child's script): the default build takes the fused kernel wherever host_api.hip allows it, ANOFOX_NARROW_FUSED=0 the
accumulate kernel + solve_narrow_kernel.  Both write every core / inference record and the refinement count of a set of
seeded batches; the parent compares them bit for bit (NaN against NaN, whatever its payload).

The batches cover p = 1..8, OLS / ridge / WLS with and without an intercept, a group count that is no multiple of the
groups per workgroup, empty groups and groups of 1 and 2 rows, non-finite rows, zero and negative weights, constant
and collinear columns, exact fits and near-rank-deficient groups (both queued for refinement), one group above the
row-splitting threshold, and inference records with and without HC errors.  The dispatch keeps the separate solve kernel
for inference records; with HC errors hc_narrow reads every group's moment record, which a fused launch would not have
written, so a wrong dispatch would show up as a mismatch.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

G_SMALL = 203      # no multiple of 4 x (groups per wavefront)
BIG_ROWS = 9000    # above seg_rows (8192 at these sizes): accumulate_segments_kernel


def _batch(p, seed, weighted, big):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(150, 400, size=G_SMALL)
    sizes[3] = 0
    sizes[10] = 1
    sizes[11] = 2
    sizes[17] = 0
    if big:
        sizes[40] = BIG_ROWS
    off = np.zeros(G_SMALL + 1, dtype=np.int64)
    off[1:] = np.cumsum(sizes)
    N = int(off[-1])
    X = rng.normal(size=(N, p)) * rng.uniform(0.5, 20.0, size=p) + rng.uniform(-50.0, 50.0, size=p)
    beta = rng.normal(size=p)
    y = X @ beta + 3.0 + rng.normal(size=N)
    w = rng.uniform(0.1, 4.0, size=N) if weighted else None
    for g in range(G_SMALL):
        lo, hi = int(off[g]), int(off[g + 1])
        if hi - lo < 8:
            continue
        kind = g % 9
        if kind == 1:                                   # non-finite rows
            X[lo + 2, 0] = np.nan
            y[lo + 5] = np.inf
            X[lo + 7, p - 1] = -np.inf
        elif kind == 2:                                 # a constant column
            X[lo:hi, p - 1] = 4.25
        elif kind == 3 and p >= 2:                      # exactly collinear columns
            X[lo:hi, 1] = 2.0 * X[lo:hi, 0] - 1.0
        elif kind == 4:                                 # exact fit: queued (RSS cancels)
            y[lo:hi] = X[lo:hi] @ beta + 3.0
        elif kind == 5 and p >= 2:                      # nearly collinear: small pivot, queued
            X[lo:hi, 1] = X[lo:hi, 0] + 1e-7 * rng.normal(size=hi - lo)
        elif kind == 6 and weighted:                    # zero and negative weights drop rows
            w[lo:lo + 4] = 0.0
            w[lo + 4:lo + 6] = -1.0
        elif kind == 7:                                 # every row of the group invalid
            y[lo:hi] = np.nan
    return off, y, [np.ascontiguousarray(X[:, j]) for j in range(p)], w


def _configs():
    out = []
    for p in range(1, 9):
        for model in ("ols", "ridge", "wls"):
            for icpt in (True, False):
                out.append(dict(p=p, model=model, icpt=icpt, inference=False, hc="none", big=(p in (3, 8))))
    for p in (2, 8):
        out.append(dict(p=p, model="ols", icpt=True, inference=True, hc="none", big=False))
        out.append(dict(p=p, model="ols", icpt=True, inference=True, hc="hc1", big=False))
        out.append(dict(p=p, model="wls", icpt=False, inference=True, hc="hc0", big=False))
    out.append(dict(p=5, model="ridge", icpt=False, inference=False, hc="none", big=False, lambda_scaling="glmnet"))
    return out


def _child(out_path):
    sys.path.insert(0, ROOT)
    import importlib
    pkg = importlib.import_module("anofox-statistics_amd")
    ctx = pkg.Context()
    res = {}
    try:
        for i, c in enumerate(_configs()):
            off, y, xs, w = _batch(c["p"], 1000 + i, c["model"] == "wls", c["big"])
            opts = pkg.RegressionOptions(fit_intercept=c["icpt"], compute_inference=c["inference"], alpha=0.7,
                                         hc_type=c["hc"], lambda_scaling=c.get("lambda_scaling", "raw"))
            core, inf = pkg.fit_batch_host(off, y, xs, w, opts.batch_options(c["model"]), ctx=ctx)
            res[f"core{i}"] = np.asarray(core)
            if inf is not None:
                res[f"inf{i}"] = np.asarray(inf)
            res[f"refined{i}"] = np.array([ctx.last_refine_count()])
    finally:
        ctx.close()
    np.savez(out_path, **res)


def _same_bits(a, b):
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))


@pytest.mark.gpu
def test_fused_solve_matches_separate_solve_kernel(tmp_path):
    runs = {}
    for name, fused in (("fused", "1"), ("separate", "0")):
        out = tmp_path / f"{name}.npz"
        env = dict(os.environ, ANOFOX_NARROW_FUSED=fused)
        subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], env=env, check=True, timeout=600)
        runs[name] = np.load(out)
    a, b = runs["fused"], runs["separate"]
    assert sorted(a.files) == sorted(b.files)
    bad = [k for k in a.files if not _same_bits(a[k], b[k])]
    assert not bad, f"records differ between the fused and the separate solve: {bad}"
    # the batches do exercise the refinement queue
    assert sum(int(a[k][0]) for k in a.files if k.startswith("refined")) > 0


if __name__ == "__main__":
    _child(sys.argv[1])
