"""The cases of the mixed-model tests, shared by the CPU tier (the header's host build) and the GPU tier: calls in the library's
layout (panel_level_offsets, level_row_offsets, y, x_cols), their dense references (tests/glmm_restate.py, computed once per
process and never changed), and the comparison with its bounds."""
import json
import os
import struct

import numpy as np

import glmm_restate as R

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = json.load(open(os.path.join(HERE, "golden", "glmm", "fixtures.json")))
REC_NAMES = ("intercept", "var_group", "var_residual", "icc", "log_likelihood", "aic", "bic", "deviance", "n_observations", "n_groups",
             "iterations", "converged", "status")

# 100 x the largest scaled errors measured against the restatement, each tier from its own record (docs/PARITY.md, "Linear mixed
# models"): beta and se relative to the largest |beta| (se) of the panel and divided by the condition number of X'V^-1 X;
# var_group, var_residual and the BLUPs relative and multiplied by the curvature of l in log theta (floored at 1); l relative.
CPU_BOUNDS = {"beta": 9.7e-14, "se": 2.1e-13, "var_group": 7.6e-11, "var_residual": 2.4e-11, "ell": 7.5e-12, "blup": 2.2e-10}
GPU_BOUNDS = {"beta": 1.6e-13, "se": 2.1e-13, "var_group": 6.3e-11, "var_residual": 9.3e-12, "ell": 7.5e-12, "blup": 6.5e-11}
# 100 x the largest movement of a field when the levels of the 15 x 6 panel are permuted, measured on the GPU over the
# permutations of tests/test_gpu_glmm.py (docs/PARITY.md): the same scaling as above
PERMUTE_BOUNDS = {"beta": 2.2e-15, "var_group": 1.9e-13, "var_residual": 9.4e-14, "blup": 1.7e-13}


def panel(sizes, p, seed, sigma_b=1.0, sigma_e=0.7, nan_rows=0):
    """One panel: level l has sizes[l] rows; y = 1 + 0.5 sum x + b_l + e.  -> (sizes, y, X[n, p])"""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, np.int64)
    n = int(sizes.sum())
    X = rng.normal(size=(n, p))
    b = np.repeat(sigma_b * rng.normal(size=len(sizes)), sizes)
    y = 1.0 + 0.5 * X.sum(axis=1) / np.sqrt(p) + b + sigma_e * rng.normal(size=n)
    for i in rng.choice(n, size=nan_rows, replace=False) if nan_rows else []:
        if i % 2:
            y[i] = np.nan
        else:
            X[i, i % p] = np.nan
    return sizes, y, X


def fixture_panel(name, scale=1.0):
    d = FIXTURES[name]
    g = np.asarray(d["group"])
    sizes = np.bincount(g)
    return sizes, scale * np.asarray(d["y"], float), np.asarray(d["x"], float)[:, None]


def make_call(panels, fit_intercept=True, reml=True):
    """panels: a list of (sizes, y, X) with the same p -> the call."""
    p = panels[0][2].shape[1]
    plo, lro = [0], [0]
    for sizes, _, _ in panels:
        for s in sizes:
            lro.append(lro[-1] + int(s))
        plo.append(plo[-1] + len(sizes))
    y = np.concatenate([q[1] for q in panels]) if panels else np.zeros(0)
    X = np.concatenate([q[2] for q in panels]) if panels else np.zeros((0, p))
    return dict(plo=np.asarray(plo, np.int64), lro=np.asarray(lro, np.int64), y=np.ascontiguousarray(y),
                x_cols=[np.ascontiguousarray(X[:, j]) for j in range(p)], p=p, fit_intercept=bool(fit_intercept), reml=bool(reml))


SIZES_WAVE = (1, 1, 2, 3, 7, 63, 64, 65, 130)
LEVEL_COUNTS = (2, 3, 63, 64, 65, 257, 1025)
WIDTHS = (1, 3, 8, 9, 32)


def calls():
    """name -> call; every case the issue lists that has a dense reference"""
    out = {}
    for reml in (True, False):
        tag = "reml" if reml else "ml"
        out["fixtures-" + tag] = make_call([fixture_panel("sql_panel"), fixture_panel("flat_panel"), fixture_panel("shrink_panel"),
                                            fixture_panel("sql_panel", 2.0)], True, reml)
        out["level-sizes-" + tag] = make_call([panel(SIZES_WAVE, 3, 11), panel(SIZES_WAVE[::-1], 3, 12)], True, reml)
    out["level-counts"] = make_call([panel(np.resize([1, 2, 2], L) if L > 65 else np.resize([2, 3, 4], L), 1, 20 + L) for L in LEVEL_COUNTS])
    for p in WIDTHS:
        for icpt in (True, False):
            out["p%d-%s" % (p, "icpt" if icpt else "noicpt")] = make_call([panel(np.resize([5, 8, 11], 12), p, 40 + p),
                                                                              panel(np.resize([9, 6], 7 + p // 4), p, 41 + p)], icpt, icpt)
    nan = panel((6, 9, 70, 5, 33, 8), 3, 77, nan_rows=20)
    nan[1][6:15] = np.nan   # level 1 is empty after dropping its rows
    out["nan-rows"] = make_call([nan, panel((4, 4, 5), 3, 78, nan_rows=3)])
    return out


_REF = {}


def reference(name, call):
    """per panel the restatement's dict, or a status; computed once"""
    if name not in _REF:
        refs = []
        for g in range(len(call["plo"]) - 1):
            l0, l1 = call["plo"][g], call["plo"][g + 1]
            r0, r1 = call["lro"][l0], call["lro"][l1]
            levels = np.repeat(np.arange(l1 - l0), np.diff(call["lro"][l0:l1 + 1]))
            refs.append(R.fit_panel(call["y"][r0:r1], [c[r0:r1] for c in call["x_cols"]], levels, call["fit_intercept"], call["reml"]))
        _REF[name] = refs
    return _REF[name]


def host_input(call, waves=0, max_iterations=100, tolerance=1e-8, compute_inference=1, zq=1.959963984540054):
    head = [waves, int(call["fit_intercept"]), int(call["reml"]), max_iterations, tolerance, compute_inference, zq, len(call["plo"]) - 1,
            len(call["lro"]) - 1, call["p"], len(call["y"])]
    vals = np.concatenate([np.asarray(head, float), call["plo"].astype(float), call["lro"].astype(float), call["y"]] +
                          [c for c in call["x_cols"]])
    return struct.pack("%dd" % len(vals), *vals)


def check(call, refs, rec, inf, ranef, level_n, errs, bounds):
    """Compares every panel of a call with its reference; errs collects the largest scaled error per field.  -> (compared, left out)"""
    p, c0 = call["p"], 1 if call["fit_intercept"] else 0
    rec, inf = np.asarray(rec).reshape(-1, p + 13), np.asarray(inf).reshape(-1, 5 * p + 1)
    compared = left = 0
    for g, ref in enumerate(refs):
        l0, l1 = call["plo"][g], call["plo"][g + 1]
        r, b, ln = rec[g], np.asarray(ranef[l0:l1]), np.asarray(level_n[l0:l1])
        if not isinstance(ref, dict):
            assert r[p + 12] == ref and np.all(np.isnan(r[:p + 12])) and np.all(np.isnan(b)) and np.all(np.isnan(inf[g])), (g, ref, r)
            continue
        assert r[p + 12] == 0, (g, r)
        if ref["cond"] > 1e10:
            left += 1
            continue
        compared += 1
        beta = np.concatenate([[r[p]] if c0 else [], r[:p]])
        se = np.concatenate([[inf[g, 5 * p]] if c0 else [], inf[g, :p]])
        curv = max(ref["curvature"], 1.0) if ref["curvature"] == ref["curvature"] else 1.0
        e = {"beta": np.max(np.abs(beta - ref["beta"])) / np.max(np.abs(ref["beta"])) / ref["cond"],
             "se": np.max(np.abs(se - ref["se"])) / np.max(np.abs(ref["se"])) / ref["cond"],
             "var_residual": abs(r[p + 2] / ref["sigma2"] - 1.0) * curv,
             "ell": abs(r[p + 4] - ref["ell"]) / max(abs(ref["ell"]), 1.0)}
        assert r[p + 8] == ref["n"] and r[p + 9] == ref["n_groups"], (g, r[p + 8:p + 10], ref["n"], ref["n_groups"])
        assert np.array_equal(ln > 0, np.isfinite(b)) and int(np.sum(ln)) == ref["n"]
        got = b[ln > 0]
        if ref["theta"] == 0.0:
            assert r[p + 1] == 0.0 and r[p + 3] == 0.0 and np.all(got == 0.0) and r[p + 11] == 1, (g, r)
        elif not ref["converged"]:
            assert r[p + 11] == 0 and abs(r[p + 1] / r[p + 2] / R.THETA_HI - 1.0) <= 1e-12, (g, r)
        else:
            assert r[p + 11] == 1, (g, r)
            e["var_group"] = abs(r[p + 1] / ref["var_group"] - 1.0) * curv
            e["blup"] = np.max(np.abs(got - ref["blup"])) / np.max(np.abs(ref["blup"])) * curv
            K = ref["K"]
            assert abs(r[p + 5] - (2 * K - 2 * r[p + 4])) <= 1e-9 * abs(r[p + 5]) and r[p + 7] == -2 * r[p + 4]
            assert abs(r[p + 6] - (K * np.log(ref["n"]) - 2 * r[p + 4])) <= 1e-9 * abs(r[p + 6])
        for k, v in e.items():
            errs[k] = max(errs.get(k, 0.0), float(v))
            assert v <= bounds[k], "panel %d: %s error %.3e above %.1e" % (g, k, v, bounds[k])
    return compared, left
