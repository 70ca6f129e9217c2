"""CPU tier of the grouped elastic net: a NumPy covariance-mode coordinate-descent reference of the contract in DESIGN.md §1
("Elastic net"), checked against closed forms (and scikit-learn where it is installed); the option parser; the C / ctypes
layouts of the two option structs; the no-device failure of the new entry points."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT, import_pkg


def _soft(z, t):
    return np.sign(z) * max(abs(z) - t, 0.0)


def en_moments(y, X, fit_intercept):
    """Row filter, constant-column test, (C, c, S_yy, ybar, xbar, n, nonconst) of the contract."""
    y = np.asarray(y, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64).reshape(len(y), -1)
    ok = np.isfinite(y) & np.all(np.isfinite(X), axis=1)
    y, X = y[ok], X[ok]
    n = len(y)
    if n == 0:
        return None
    nonconst = np.any(np.abs(X - X[0]) >= 1e-10, axis=0)
    if fit_intercept:
        xbar, ybar = X.mean(axis=0), y.mean()
        Xc, yc = X - xbar, y - ybar
    else:
        xbar, ybar = np.zeros(X.shape[1]), 0.0
        Xc, yc = X, y
    return dict(C=Xc.T @ Xc, c=Xc.T @ yc, syy=float(yc @ yc), ybar=float(y.mean()), xbar=xbar, n=n, nonconst=nonconst,
                cyy=float(((y - y.mean()) ** 2).sum()), X=X, y=y)


def en_lambda(m, alpha, lambda_scaling):
    if lambda_scaling == "glmnet":
        return m["n"] * alpha / np.sqrt(m["cyy"] / m["n"])
    return alpha


def en_cd(Cm, c, lam, l1, active, tol, max_iter, syy):
    """Cyclic coordinate descent from b = 0; returns (b, sweeps, converged)."""
    p = len(c)
    b = np.zeros(p)
    pen1 = lam * l1 if l1 > 0 else 0.0
    pen2 = lam * (1 - l1) if l1 < 1 else 0.0
    thresh = tol * np.sqrt(syy)
    for it in range(1, max_iter + 1):
        dmax = 0.0
        for j in range(p):
            if not active[j]:
                continue
            z = c[j] - Cm[j] @ b + Cm[j, j] * b[j]
            bn = _soft(z, pen1) / (Cm[j, j] + pen2)
            dmax = max(dmax, np.sqrt(Cm[j, j]) * abs(bn - b[j]))
            b[j] = bn
        if dmax <= thresh:
            return b, it, True
    return b, max_iter, False


def en_reference(y, X, alpha=1.0, l1_ratio=0.5, fit_intercept=True, lambda_scaling="raw", tol=1e-15, max_iter=100000):
    """Core record {coef[p], intercept, r2, adj_r2, rse, n, status} of one group, as the batch path defines it."""
    X = np.asarray(X, dtype=np.float64).reshape(len(y), -1)
    p = X.shape[1]
    rec = np.full(p + 6, np.nan)
    if len(y) < 2:
        rec[p + 5] = 100
        return rec
    if not alpha >= 0:
        rec[p + 5] = 4
        return rec
    if not 0 <= l1_ratio <= 1:
        rec[p + 5] = 5
        return rec
    m = en_moments(y, X, fit_intercept)
    if m is None:
        rec[p + 5] = 10
        return rec
    n, act = m["n"], m["nonconst"]
    k = int(act.sum())
    if k == 0:
        if not fit_intercept:
            rec[p + 5] = 6
            return rec
        rec[p:p + 6] = [m["ybar"], 0.0, 0.0, np.sqrt(m["cyy"] / (n - 1)), n, 0]
        return rec
    if n < k + (1 if fit_intercept else 0):
        rec[p + 5] = 6
        return rec
    lam = en_lambda(m, alpha, lambda_scaling)
    b, _, _ = en_cd(m["C"], m["c"], lam, l1_ratio, act, tol, max_iter, m["syy"])
    r = m["y"] - m["X"] @ b
    b0 = m["ybar"] - m["xbar"] @ b if fit_intercept else 0.0
    rss = float(((r - b0) ** 2).sum())
    tss = m["syy"]
    df = n - (k + (1 if fit_intercept else 0))
    r2 = 1 - rss / tss
    rec[:p] = np.where(act, b, np.nan)
    rec[p] = b0 if fit_intercept else np.nan
    rec[p + 1:p + 6] = [r2, 1 - (1 - r2) * (n - (1 if fit_intercept else 0)) / df, np.sqrt(rss / df), n, 0]
    return rec


def lambda_max(y, X, l1_ratio, fit_intercept=True):
    m = en_moments(y, X, fit_intercept)
    return float(np.max(np.abs(m["c"][m["nonconst"]]))) / l1_ratio


def _data(n, p, seed):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, p))
    y = X @ rng.normal(size=p) + 0.5 + 0.3 * rng.normal(size=n)
    return y, X


# ---- the reference against closed forms ----

@pytest.mark.parametrize("fit_intercept", [True, False])
def test_l1_zero_is_the_ridge_solve(fit_intercept):
    y, X = _data(80, 5, 1)
    lam = 3.0
    rec = en_reference(y, X, alpha=lam, l1_ratio=0.0, fit_intercept=fit_intercept)
    m = en_moments(y, X, fit_intercept)
    b = np.linalg.solve(m["C"] + lam * np.eye(5), m["c"])
    assert np.allclose(rec[:5], b, rtol=1e-12, atol=1e-13)


def test_orthonormal_design_gives_the_soft_threshold():
    rng = np.random.default_rng(2)
    Q, _ = np.linalg.qr(rng.normal(size=(50, 4)))
    Q -= Q.mean(axis=0)
    Q, _ = np.linalg.qr(Q)          # centred orthonormal columns: C = I
    y = Q @ np.array([3.0, -0.2, 1.0, 0.05]) + 0.01 * rng.normal(size=50)
    lam, l1 = 0.5, 0.7
    rec = en_reference(y, Q, alpha=lam, l1_ratio=l1)
    m = en_moments(y, Q, True)
    expect = np.array([_soft(cj, lam * l1) for cj in m["c"]]) / (1 + lam * (1 - l1))
    assert np.allclose(rec[:4], expect, atol=1e-13)
    assert rec[1] == 0.0 and rec[3] == 0.0


@pytest.mark.parametrize("l1", [0.3, 1.0])
def test_lambda_beyond_lambda_max_gives_zero(l1):
    y, X = _data(60, 6, 3)
    lm = lambda_max(y, X, l1)
    rec = en_reference(y, X, alpha=lm * 1.0001, l1_ratio=l1)
    assert np.all(rec[:6] == 0.0) and np.isclose(rec[6], np.mean(y), rtol=1e-14)
    rec = en_reference(y, X, alpha=lm * 0.9, l1_ratio=l1)
    assert np.any(rec[:6] != 0.0)


def test_alpha_zero_is_ols():
    y, X = _data(70, 4, 4)
    rec = en_reference(y, X, alpha=0.0, l1_ratio=0.5)
    A = np.column_stack([X, np.ones(70)])
    beta = np.linalg.lstsq(A, y, rcond=None)[0]
    assert np.allclose(rec[:4], beta[:4], rtol=1e-10) and np.isclose(rec[4], beta[4], rtol=1e-10)


def test_reference_agrees_with_scikit_learn():
    lm = pytest.importorskip("sklearn.linear_model")
    y, X = _data(120, 6, 5)
    n = len(y)
    for lam, l1 in ((5.0, 0.5), (20.0, 1.0), (1.0, 0.2)):
        rec = en_reference(y, X, alpha=lam, l1_ratio=l1)
        sk = lm.ElasticNet(alpha=lam / n, l1_ratio=l1, fit_intercept=True, tol=1e-14, max_iter=100000).fit(X, y)
        assert np.allclose(rec[:6], sk.coef_, atol=1e-8) and np.isclose(rec[6], sk.intercept_, atol=1e-8)


def test_statuses_and_shortcut():
    y, X = _data(30, 3, 6)
    assert en_reference(y, X, alpha=-1.0)[3 + 5] == 4
    assert en_reference(y, X, l1_ratio=1.5)[3 + 5] == 5
    assert en_reference(np.full(5, np.nan), np.ones((5, 3)))[3 + 5] == 10
    assert en_reference(y[:3], X[:3])[3 + 5] == 6
    rec = en_reference(y, np.ones((30, 3)))
    assert rec[8] == 0 and np.all(np.isnan(rec[:3])) and np.isclose(rec[3], y.mean())
    assert rec[4] == 0 and rec[5] == 0 and np.isclose(rec[6], np.std(y, ddof=1))
    assert en_reference(y, np.ones((30, 3)), fit_intercept=False)[8] == 6


# ---- options ----

def test_parse_elasticnet_options():
    pkg = import_pkg()
    o = pkg.parse_elasticnet_options(None)
    assert (o.alpha, o.l1_ratio, o.fit_intercept, o.max_iterations, o.tolerance, o.lambda_scaling) == (1.0, 0.5, True, 1000, 1e-6, "raw")
    o = pkg.parse_elasticnet_options({"LAMBDA": 0.1, "Alpha": 0.5, "L1_RATIO": 0.25, "intercept": False, "MAX_ITER": 7,
                                      "tol": 1e-9, "lambda_scaling": "GLMNET", "unknown_key": 3})
    assert (o.alpha, o.l1_ratio, o.fit_intercept, o.max_iterations, o.tolerance, o.lambda_scaling) == (0.5, 0.25, False, 7, 1e-9, "glmnet")
    o = pkg.parse_elasticnet_options({"lambda": 0.1, "fit_intercept": 0, "max_iterations": 5, "tolerance": 1e-3})
    assert (o.alpha, o.fit_intercept, o.max_iterations, o.tolerance) == (0.1, False, 5, 1e-3)
    with pytest.raises(pkg.InvalidInputException, match="Invalid lambda_scaling: 'foo'. Valid values are 'raw', 'glmnet'"):
        pkg.parse_elasticnet_options({"lambda_scaling": "foo"})
    with pytest.raises(pkg.InvalidInputException, match="Cannot convert value of type STR to boolean"):
        pkg.parse_elasticnet_options({"intercept": "yes"})
    with pytest.raises(pkg.InvalidInputException, match="constant expression"):
        pkg.parse_elasticnet_options([1, 2])
    b = pkg.parse_elasticnet_options({"alpha": 2.0}).batch_options()
    assert b.alpha == 2.0 and b.l1_ratio == 0.5 and b.max_iterations == 1000 and b.fit_intercept


# ---- layouts ----

def test_option_struct_layouts():
    abi = import_pkg("_abi")
    E, B = abi.AnofoxElasticNetOptions, abi.AnofoxHipElasticNetBatchOptions
    assert C.sizeof(E) == 40
    assert [getattr(E, f).offset for f in ("alpha", "l1_ratio", "fit_intercept", "max_iterations", "tolerance", "lambda_scaling")] == [0, 8, 16, 20, 24, 32]
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "anofox_stats_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(AnofoxElasticNetOptions), offsetof(AnofoxElasticNetOptions, alpha),
         offsetof(AnofoxElasticNetOptions, l1_ratio), offsetof(AnofoxElasticNetOptions, fit_intercept),
         offsetof(AnofoxElasticNetOptions, max_iterations), offsetof(AnofoxElasticNetOptions, tolerance),
         offsetof(AnofoxElasticNetOptions, lambda_scaling));
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(AnofoxHipElasticNetBatchOptions),
         offsetof(AnofoxHipElasticNetBatchOptions, fit_intercept), offsetof(AnofoxHipElasticNetBatchOptions, alpha),
         offsetof(AnofoxHipElasticNetBatchOptions, l1_ratio), offsetof(AnofoxHipElasticNetBatchOptions, max_iterations),
         offsetof(AnofoxHipElasticNetBatchOptions, tolerance), offsetof(AnofoxHipElasticNetBatchOptions, lambda_scaling));
  return 0;
}
'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.check_output([exe]).decode().split("\n")
    assert [int(v) for v in out[0].split()] == [40, 0, 8, 16, 20, 24, 32]
    got = [int(v) for v in out[1].split()]
    assert got == [C.sizeof(B)] + [getattr(B, f).offset for f in ("fit_intercept", "alpha", "l1_ratio", "max_iterations",
                                                                      "tolerance", "lambda_scaling")]


# ---- no device ----

def test_entry_points_fail_without_a_device():
    if os.path.exists("/dev/kfd"):
        pytest.skip("checks the no-device path: a GPU is present")
    pkg = import_pkg()
    with pytest.raises(pkg.InvalidInputException, match="no HIP device"):
        pkg.elasticnet_fit([1.0, 2.0, 3.5], [[1.0, 2.0, 3.0]])
    o = pkg.parse_elasticnet_options(None).batch_options()
    with pytest.raises(pkg.AnofoxStatsError, match="no HIP device"):
        pkg.elasticnet_fit_batch_host([0, 3], [1.0, 2.0, 3.5], [[1.0, 2.0, 3.0]], o)


def test_argument_errors_precede_device_use():
    pkg = import_pkg()
    with pytest.raises(pkg.InvalidInputException, match="Invalid alpha parameter: -1 \\(must be >= 0\\)"):
        pkg.elasticnet_fit([1.0, 2.0, 3.5], [[1.0, 2.0, 3.0]], {"alpha": -1.0})
    with pytest.raises(pkg.InvalidInputException, match="Invalid L1 ratio: 2 \\(must be in \\[0, 1\\]\\)"):
        pkg.elasticnet_fit([1.0, 2.0, 3.5], [[1.0, 2.0, 3.0]], {"l1_ratio": 2.0})
    with pytest.raises(pkg.InvalidInputException, match="Dimension mismatch"):
        pkg.elasticnet_fit([1.0, 2.0, 3.5], [[1.0, 2.0]])


# ---- the DuckDB glue (duckdb_shim/elasticnet_agg_hip.cpp) through its test driver ----

def test_glue_feature_count_errors_name_the_counts():
    """elasticnet_fit_agg: one state given a 2-feature row and then a 3-feature row, and a 2-feature state combined into a
    3-feature state — the texts of elasticnet_aggregate.cpp, with the counts.  Both are thrown before Finalize: no device."""
    import ctypes as C
    import_pkg()
    lib = C.CDLL(os.path.join(ROOT, "anofox-statistics_amd", "duckdb_shim", "libanofox_elasticnet_glue_capi.so"))
    lib.en_open.restype = C.c_void_p
    lib.en_open.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_char_p]
    lib.en_close.argtypes = [C.c_void_p]
    lib.en_feature_count_errors.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
    msg, update, combine = (C.create_string_buffer(512) for _ in range(3))
    q = lib.en_open(b"elasticnet_fit_agg", None, 0, msg)
    assert q, msg.value.decode()
    lib.en_feature_count_errors(q, update, combine)
    lib.en_close(q)
    assert update.value.decode() == "Inconsistent feature count: expected 2, got 3"
    assert combine.value.decode() == "Cannot combine states with different feature counts: 2 vs 3"


# ---- the DuckDB glue compiles cleanly against the stand-in of DuckDB's headers ----

def test_glue_compiles_warning_free():
    shim = os.path.join(ROOT, "anofox-statistics_amd", "duckdb_shim")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "tests", "tools", "duckdb_stub"), "-I", os.path.join(ROOT, "include"), "-I", shim,
                           os.path.join(shim, "elasticnet_agg_hip.cpp")])


def test_row_glue_header_stands_alone(tmp_path):
    """duckdb_shim/row_glue.hpp included alone: it leans on nothing a particular .cpp included before it."""
    shim = os.path.join(ROOT, "anofox-statistics_amd", "duckdb_shim")
    src = tmp_path / "row_glue_alone.cpp"
    src.write_text('#include "row_glue.hpp"\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror",
                        "-I", os.path.join(ROOT, "tests", "tools", "duckdb_stub"), "-I", os.path.join(ROOT, "include"), "-I", shim, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
