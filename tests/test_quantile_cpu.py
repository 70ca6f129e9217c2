"""Quantile regression without a GPU: the golden cases (tests/golden/quantile/cases.json, written by
tests/golden/make_quantile_cases.py from scipy's HiGHS) against the certificate of tests/quantile_restate.py; the solve header
csrc/quantile_solve.h compiled as plain C++ under ASan / UBSan behind a stand-alone main (tests/tools/quantile_solve_host.cpp)
over the same cases with the GPU test's assertions; the options parser; the C ABI's struct layouts as literal numbers worked
out from the declarations of the reference's header (AnofoxQuantileOptions: double @0, bool @8, uint32 @12, double @16 = 24
bytes; AnofoxQuantileFitResultCore: six 8-byte fields = 48).

The DuckDB glue of this family is not built, so there is no glue test here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import quantile_restate as qr
from conftest import ROOT, import_pkg


@pytest.fixture(scope="module")
def cases():
    return qr.load_cases()


def check_record(c, rec, its, what):
    """The assertions both solvers (host build, GPU) have to meet on a golden case; -> whether the coefficients were compared."""
    X, y, tau, icpt = c["X"], c["y"], c["tau"], c["fit_intercept"]
    p = X.shape[1]
    status = qr.rule_status(X, y, tau, icpt)
    assert rec[p + 5] == status, f"{what}: status {rec[p + 5]} != {status}"
    if status != 0:
        assert np.isnan(rec[:p + 5]).all(), what
        return False
    assert its >= 0, f"{what}: the iteration bound stopped the fit ({its})"
    b, b0 = rec[:p], rec[p]
    assert np.isnan(b0) == (not icpt), what
    assert rec[p + 1] == tau and rec[p + 4] == len(y), what
    loss = qr.pinball_loss(X, y, tau, b, b0)
    # loss <= golden (1 + 1e-9).  Only where the golden fit interpolates (loss <= 1e-12 max|y|: n = k, both losses are the
    # ~1e-15 rounding of an exact 0) the rounding of evaluating the residuals at all in binary64 is allowed on top:
    # (k + 2) 2^-52 per row of |y_i| + |a_i|'|beta|
    noise = 0.0
    if c["loss"] <= 1e-12 * np.max(np.abs(y)):
        A = qr.design(X, icpt)
        beta = np.concatenate([[b0], b]) if icpt else b
        noise = (A.shape[1] + 2) * 2.0 ** -52 * float(np.sum(np.abs(y) + np.abs(A) @ np.abs(beta)))
    assert loss <= c["loss"] * (1 + 1e-9) + noise, f"{what}: loss {loss!r} > golden {c['loss']!r}"
    assert abs(rec[p + 2] - loss) <= 1e-9 * max(loss, 1e-300) + 1e-12 * np.max(np.abs(y)), f"{what}: record loss {rec[p + 2]!r} vs {loss!r}"
    cert = qr.certify(X, y, tau, icpt, b, b0)
    if cert["decided"]:                    # |Z| = k and A_Z non-singular (aliased tables have a singular A_Z: no certificate)
        assert cert["optimal"], f"{what}: not optimal {cert}"
    if not c["unique"]:
        return False
    assert cert["decided"] and cert["optimal"], f"{what}: {cert}"
    scale = max(1.0, np.max(np.abs(c["b"])))
    assert np.max(np.abs(b - c["b"])) <= 1e-9 * scale, f"{what}: coefficients off by {np.max(np.abs(b - c['b'])) / scale:.3g}"
    if icpt:
        assert abs(b0 - c["b0"]) <= 1e-9 * max(scale, abs(c["b0"])), f"{what}: intercept off by {abs(b0 - c['b0']):.3g}"
    return True


def test_certificate_accepts_golden_and_rejects_a_moved_coefficient(cases):
    n_unique = 0
    for c in cases:
        cert = qr.certify(c["X"], c["y"], c["tau"], c["fit_intercept"], c["b"], c["b0"])
        if cert["decided"]:
            assert cert["optimal"], c["name"]
        assert qr.pinball_loss(c["X"], c["y"], c["tau"], c["b"], c["b0"]) <= c["loss"] * (1 + 1e-12) + 1e-300
        if c["unique"]:
            n_unique += 1
            assert cert["decided"] and cert["strict"], c["name"]
            b = c["b"].copy()
            b[0] += 1e-3
            moved = qr.certify(c["X"], c["y"], c["tau"], c["fit_intercept"], b, c["b0"])
            assert not (moved["decided"] and moved["optimal"]), c["name"]
            assert qr.pinball_loss(c["X"], c["y"], c["tau"], b, c["b0"]) > c["loss"]
    gauss = [c for c in cases if c["name"].startswith("gauss")]
    assert len(gauss) == 180 and all(c["unique"] for c in gauss)      # every Gaussian case is a single non-degenerate vertex


def test_golden_agrees_with_scipy(cases):
    opt = pytest.importorskip("scipy.optimize")
    for c in cases[::7]:
        A = qr.design(c["X"], c["fit_intercept"])
        n, k = A.shape
        cost = np.concatenate([np.zeros(k), np.full(n, c["tau"]), np.full(n, 1.0 - c["tau"])])
        res = opt.linprog(cost, A_eq=np.hstack([A, np.eye(n), -np.eye(n)]), b_eq=c["y"],
                          bounds=[(None, None)] * k + [(0, None)] * (2 * n), method="highs-ds")
        assert res.status == 0
        assert abs(res.fun - c["loss"]) <= 1e-8 * max(1.0, abs(c["loss"])), c["name"]


def test_restatement_rules():
    rng = np.random.default_rng(5)
    X, y = rng.normal(size=(12, 3)), rng.normal(size=12)
    assert qr.rule_status(X, y, 0.5, True) == 0
    for tau in (0.0, 1.0, -0.1, 1.5, float("nan")):
        assert qr.rule_status(X, y, tau, True) == 1
    assert qr.rule_status(X[:1], y[:1], 0.5, False) == 100
    assert qr.rule_status(X, np.full(12, np.nan), 0.5, True) == 10
    assert qr.rule_status(X[:3], y[:3], 0.5, True) == 6 and qr.rule_status(X[:3], y[:3], 0.5, False) == 0   # equality allowed
    assert qr.rule_status(X[:4], y[:4], 0.5, True) == 0
    y2 = y.copy()
    y2[:10] = np.inf
    assert qr.rule_status(X, y2, 0.5, False) == 6                        # two valid rows, three columns
    assert qr.pinball_loss(np.array([[0.0], [0.0]]), np.array([1.0, -1.0]), 0.9, [0.0], None) == pytest.approx(0.9 + 0.1)


def test_option_parser():
    pkg = import_pkg()
    o = pkg.parse_quantile_options(None)
    assert (o.tau, o.fit_intercept, o.max_iterations, o.tolerance) == (0.5, True, 1000, 1e-6)
    o = pkg.parse_quantile_options({"TAU": 0.9, "Intercept": False, "max_iter": 7, "tol": 1e-8, "alpha": 3.0})
    assert (o.tau, o.fit_intercept, o.max_iterations, o.tolerance) == (0.9, False, 7, 1e-8)
    assert pkg.parse_quantile_options({"fit_intercept": False, "tau": 1}).tau == 1.0       # the range is the fit's to report
    with pytest.raises(pkg.InvalidInputException, match="must be a constant expression"):
        pkg.parse_quantile_options([("tau", 0.5)])
    with pytest.raises(pkg.InvalidInputException, match="out of range for UINTEGER"):
        pkg.parse_quantile_options({"max_iterations": -1})
    b = pkg.parse_quantile_options({"tau": 0.25}).batch_options()
    assert (b.tau, b.fit_intercept, b.max_iterations, b.tolerance) == (0.25, True, 1000, 1e-6)
    for name in ("anofox_stats_quantile_fit_predict_agg", "quantile_fit_predict_agg", "anofox_stats_quantile_fit", "quantile_fit"):
        assert name in pkg.SQL_FUNCTIONS


def test_abi_layout():
    abi = import_pkg("_abi")
    o, r = abi.AnofoxQuantileOptions, abi.AnofoxQuantileFitResultCore
    assert C.sizeof(o) == 24 and C.sizeof(abi.AnofoxHipQuantileBatchOptions) == 24
    assert [getattr(o, f).offset for f, _ in o._fields_] == [0, 8, 12, 16]
    assert [getattr(abi.AnofoxHipQuantileBatchOptions, f).offset for f, _ in o._fields_] == [0, 8, 12, 16]
    assert C.sizeof(r) == 48
    assert [getattr(r, f).offset for f, _ in r._fields_] == [0, 8, 16, 24, 32, 40]
    with open(os.path.join(ROOT, "include", "anofox_stats_hip.h")) as f:
        h = f.read()
    for name, cls in (("AnofoxQuantileOptions", o), ("AnofoxQuantileFitResultCore", r), ("AnofoxHipQuantileBatchOptions", o)):
        body = re.search(r"typedef struct \{([^}]*)\} " + name + ";", h).group(1)
        assert re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == [f for f, _ in cls._fields_], name
    for sym in ("anofox_quantile_fit", "anofox_free_quantile_result", "anofox_hip_quantile_record_len",
                "anofox_hip_quantile_fit_batch_device", "anofox_hip_quantile_fit_batch_host",
                "anofox_hip_quantile_fit_predict_batch_device", "anofox_hip_quantile_fit_predict_batch_host"):
        assert sym in abi.SYMBOLS and re.search(r"\b" + sym + r"\(", h), sym
    lib = abi.load()
    assert lib.anofox_hip_quantile_record_len(5) == 11
    lib.anofox_free_quantile_result(None)           # NULL-safe


def _case_text(X, y, tau, icpt, max_it=1000, rule=None):
    lines = [f"{X.shape[1]} {int(icpt)} {tau!r} {len(y)} {max_it} {len(y) if rule is None else rule}"]
    lines += [" ".join(repr(float(v)) for v in (y[i], *X[i])) for i in range(len(y))]
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module")
def host_solver(tmp_path_factory):
    """tests/tools/quantile_solve_host.cpp under ASan / UBSan: a program of its own, never loaded into python."""
    exe = str(tmp_path_factory.mktemp("qs") / "quantile_solve_host")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1",
                        os.path.join(ROOT, "tests", "tools", "quantile_solve_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(text):
        env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
        out = subprocess.run([exe], input=text, capture_output=True, text=True, env=env)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
        assert "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
        return [np.array([float(t) for t in ln.split()]) for ln in out.stdout.strip().split("\n")]
    return run


def test_host_build_of_the_solve_meets_the_gpu_assertions(cases, host_solver):
    rows = host_solver("".join(_case_text(c["X"], c["y"], c["tau"], c["fit_intercept"]) for c in cases))
    assert len(rows) == len(cases)
    compared = 0
    for c, v in zip(cases, rows):
        p = c["X"].shape[1]
        compared += check_record(c, v[:p + 6], int(v[p + 6]), c["name"])
    gauss = sum(c["name"].startswith("gauss") for c in cases)
    assert compared >= 0.95 * gauss                    # at most 5 % of the Gaussian cases may go without a coefficient comparison


def test_host_build_rules_masking_aliasing_and_the_iteration_bound(cases, host_solver):
    c = next(c for c in cases if c["name"] == "gauss p=2 icpt=1 n=64 tau=0.5")
    X, y = c["X"], c["y"]
    Xn, yn = np.vstack([X[:20], [[np.nan, 1.0]], X[20:], [[0.0, np.inf]]]), np.concatenate([y[:20], [1.0], y[20:], [2.0]])
    yn2, Xn2 = np.concatenate([yn, [np.nan]]), np.vstack([Xn, [[0.5, 0.5]]])
    Xa = np.column_stack([X[:, 0], 0.5 * X[:, 0], X[:, 1], np.full(len(y), 3.0)])   # x2 = 0.5 x1 and a constant next to the intercept
    text = (_case_text(Xn2, yn2, 0.5, True) + _case_text(X, np.full(len(y), np.nan), 0.5, True) + _case_text(X[:2], y[:2], 0.5, True) +
            _case_text(X[:1], y[:1], 0.5, False) + _case_text(X, y, 0.0, True) + _case_text(X, y, 1.0, True) +
            _case_text(X, y, float("nan"), True) + _case_text(X, y, 0.5, True, max_it=1) + _case_text(Xa, y, 0.5, True) +
            _case_text(X, y, 0.5, True, rule=1))
    r = host_solver(text)
    assert r[0][7] == 0 and r[0][6] == 64 and np.max(np.abs(r[0][:3] - np.concatenate([c["b"], [c["b0"]]]))) <= 1e-9 * max(1, np.abs(c["b"]).max())
    assert [int(v[7]) for v in r[1:7]] == [10, 6, 100, 1, 1, 1]
    for v in r[1:7]:
        assert np.isnan(v[:7]).all()
    assert r[7][7] == 0 and r[7][8] == -1 and np.isfinite(r[7][:3]).all()                    # last vertex, negated count
    a = r[8]
    assert a[9] == 0 and a[7] == 3 and a[10] >= 0                                           # rank 3 of k = 5: two artificials left
    assert (a[:5] == 0.0).sum() == 2 and abs(a[6] - c["loss"]) <= 1e-9 * c["loss"]          # aliased slots (which of a set: not fixed) exactly 0.0, the same loss
    assert r[9][7] == 100


def test_host_build_ignores_stale_scratch_of_masked_rows(cases, host_solver):
    """60 training rows and 20 prediction rows (y NaN), as every fit-predict call has them.  The tool fits each case a second
    time on scratch filled with positive stale values and ends with an error if a byte of the record or the pivot count
    differs; the result is the fit of the 60 rows alone."""
    c = next(c for c in cases if c["name"] == "gauss p=8 icpt=1 n=130 tau=0.5")
    X, y = c["X"][:80], c["y"][:80].copy()
    y[60:] = np.nan
    for tau in (0.1, 0.5, 0.9):
        both = host_solver(_case_text(X, y, tau, True) + _case_text(X[:60], y[:60], tau, True))
        assert both[0][13] == 0 and both[0][12] == 60 and both[0][14] >= 0
        assert np.array_equal(both[0], both[1])


def test_host_build_degenerate_ties_terminate(host_solver):
    """Integer y on integer x: ties and zero residuals off the basis.  The fit ends converged, and no coefficient moved by
    1e-3 does better."""
    i = np.arange(1.0, 41.0)
    X = np.column_stack([i, (i % 5)])
    y = 3.0 * i + (i % 4) - 2.0 * (i % 5)
    text = "".join(_case_text(X, y, tau, icpt) for tau in (0.1, 0.5, 0.9) for icpt in (True, False))
    rows = host_solver(text)
    k = 0
    for tau in (0.1, 0.5, 0.9):
        for icpt in (True, False):
            v = rows[k]
            k += 1
            assert v[7] == 0 and v[8] >= 0
            loss = qr.pinball_loss(X, y, tau, v[:2], v[2])
            assert abs(loss - v[4]) <= 1e-9 * max(loss, 1.0)
            for j in range(2):
                for d in (-1e-3, 1e-3):
                    b = v[:2].copy()
                    b[j] += d
                    assert qr.pinball_loss(X, y, tau, b, v[2]) >= loss * (1 - 1e-12)
