"""Bounded least squares without a GPU: the row-based restatement (tests/bls_restate.py) against the KKT conditions of the
problem, the reference's pivot regression case, OLS where no bound binds; the options parsers; the C ABI's struct layouts
as literal numbers worked out from the declarations of the reference's header (AnofoxBlsOptions: bool @0, pointer @8,
size_t @16, pointer @24, size_t @32, uint32 @40, double @48 = 56 bytes; AnofoxBlsFitResultCore: ten 8-byte fields = 80)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bls_restate as br
from conftest import ROOT, import_pkg

BOUND_SETS = [
    ("nnls", None, None),
    ("box", -1.0, 1.5),
    ("lower_only", -0.5, None),
    ("upper_only", None, 0.25),
]


@pytest.mark.parametrize("name,lower,upper", BOUND_SETS)
@pytest.mark.parametrize("fit_intercept", [False, True])
def test_restatement_satisfies_kkt(name, lower, upper, fit_intercept):
    rng = np.random.default_rng(7)
    n_bound = n_coef = 0
    for case in range(60):
        p = int(rng.integers(1, 41))
        n = int(rng.integers(p + 2, 6 * p + 41))
        y, X = br.make_case(rng, n, p)
        lo, hi = lower, upper
        if name == "box" and case % 3 == 0:       # per-column bounds
            lo, hi = rng.uniform(-2.0, 0.0, size=p), rng.uniform(0.0, 2.0, size=p)
        res = br.fit_bls(y, X, fit_intercept, lo, hi)
        assert res["status"] == 0
        worst_free, wrong = br.kkt_residuals(res, y, X, fit_intercept)
        assert worst_free <= 1e-9, (case, p, n, worst_free)
        assert wrong <= 1e-9, (case, p, n, wrong)
        b = res["coefficients"]
        assert (b >= res["lo"]).all() and (b <= res["hi"]).all()
        assert res["iterations"] <= 3 * p + 3
        assert br.input_conditions(res, y, X, fit_intercept) == []
        n_bound += int(res["n_active_constraints"])
        n_coef += p
    assert 0.05 * n_coef < n_bound < 0.95 * n_coef   # the sweep exercises bound and free coefficients alike


def test_pivot_case_of_the_reference():
    """test/sql/regression/test_bls_nnls_pivot.test restated: columns of scale 1e-3 / 1e3 / 10, no intercept, an exact fit;
    the reference asserts the coefficients rounded to three decimals."""
    y, X = br.pivot_table()
    for lower, upper in ((None, None), (0.0, None)):
        res = br.fit_bls(y, X, False, lower, upper)
        assert res["status"] == 0
        assert np.array_equal(np.round(res["coefficients"], 3), [7.0, 2.0, 0.5])
        assert res["n_active_constraints"] == 0 and res["ssr"] < 1e-12 * float(y @ y)
    ols = np.linalg.lstsq(X, y, rcond=None)[0]
    assert np.array_equal(np.round(ols, 3), [7.0, 2.0, 0.5])


@pytest.mark.parametrize("fit_intercept", [False, True])
def test_inactive_bounds_give_ols(fit_intercept):
    rng = np.random.default_rng(11)
    y, X = br.make_case(rng, 80, 6)
    res = br.fit_bls(y, X, fit_intercept, -1e3, 1e3)
    D = np.concatenate([np.ones((80, 1)), X], axis=1) if fit_intercept else X
    sol = np.linalg.lstsq(D, y, rcond=None)[0]
    np.testing.assert_allclose(res["coefficients"], sol[1:] if fit_intercept else sol, rtol=1e-10)
    assert res["n_active_constraints"] == 0
    if fit_intercept:
        assert abs(res["intercept"] - sol[0]) < 1e-9
    else:
        assert np.isnan(res["intercept"])


def test_restatement_rules():
    rng = np.random.default_rng(3)
    y, X = br.make_case(rng, 30, 3)
    assert br.fit_bls(y[:1], X[:1])["status"] == 100
    assert br.fit_bls(y, X, lower=[0.0, 1.0])["status"] == 1                 # neither 1 nor p values
    assert br.fit_bls(y, X, lower=2.0, upper=1.0)["status"] == 1
    assert br.fit_bls(y, X, lower=np.nan)["status"] == 1
    assert br.fit_bls(np.full(30, np.nan), X)["status"] == 10
    Xc = np.ones((30, 3))
    assert br.fit_bls(y, Xc, fit_intercept=False)["status"] == 6
    sc = br.fit_bls(y, Xc, fit_intercept=True)
    assert sc["status"] == 0 and np.isnan(sc["ssr"]) and sc["r_squared"] == 0.0 and np.isnan(sc["coefficients"]).all()
    assert abs(sc["intercept"] - y.mean()) < 1e-12 and sc["n_active_constraints"] == 0
    assert br.fit_bls(y[:3], X[:3], fit_intercept=True)["status"] == 6       # 3 rows < 3 columns + intercept
    assert br.fit_bls(y[:3], X[:3], fit_intercept=False)["status"] == 0      # equality allowed
    X2 = X.copy()
    X2[:, 1] = 4.0                                                           # a constant column: NaN, no flag
    r = br.fit_bls(y, X2, lower=100.0, upper=101.0)
    assert np.isnan(r["coefficients"][1]) and not r["at_lower_bound"][1] and not r["at_upper_bound"][1]
    assert r["n_active_constraints"] == 2 and set(r["coefficients"][[0, 2]]) <= {100.0, 101.0}
    rec = br.record(r)
    assert rec.shape == (15,) and rec[3 + 5] == 0 and rec[3 + 4] == 2


def test_option_parsers():
    pkg = import_pkg()
    o = pkg.parse_bls_options(None)
    assert (o.fit_intercept, o.lower_bound, o.upper_bound, o.max_iterations, o.tolerance) == (False, None, None, 1000, 1e-10)
    o = pkg.parse_bls_options({"Intercept": True, "LOWER": -1, "upper_bound": 2.5, "max_iter": 7, "tol": 1e-8, "alpha": 3.0})
    assert (o.fit_intercept, o.lower_bound, o.upper_bound, o.max_iterations, o.tolerance) == (True, -1.0, 2.5, 7, 1e-8)
    o = pkg.parse_nnls_options({"lower": -5.0, "upper_bound": 1.0, "fit_intercept": True, "max_iterations": 9, "tolerance": 1e-7})
    assert (o.fit_intercept, o.lower_bound, o.upper_bound, o.max_iterations, o.tolerance) == (True, None, None, 9, 1e-7)
    o = pkg.parse_bls_predict_options({"lower_bound": 0.0, "confidence": 0.9, "null_policy": "DROP_Y_ZERO_X"})
    assert (o.lower_bound, o.confidence_level, o.null_policy) == (0.0, 0.9, "drop_y_zero_x")
    assert pkg.parse_bls_predict_options(None).confidence_level == 0.95
    with pytest.raises(pkg.InvalidInputException, match="Invalid null_policy: 'keep'"):
        pkg.parse_bls_predict_options({"null_policy": "keep"})
    with pytest.raises(pkg.InvalidInputException, match="must be a constant expression"):
        pkg.parse_bls_options([("lower", 1)])
    with pytest.raises(pkg.InvalidInputException, match="out of range for UINTEGER"):
        pkg.parse_bls_options({"max_iterations": -1})
    b = pkg.parse_bls_options({"lower": -1.0, "upper": [1.0, 2.0, 3.0]}).batch_options()
    assert (b.lower_bounds_len, b.upper_bounds_len, b.lower_bounds[0], b.upper_bounds[2]) == (1, 3, -1.0, 3.0)
    b = pkg.parse_nnls_options(None).batch_options()
    assert (b.lower_bounds_len, b.upper_bounds_len, bool(b.lower_bounds), bool(b.upper_bounds)) == (0, 0, False, False)
    for name in ("anofox_stats_bls_fit_agg", "bls_fit_agg", "anofox_stats_nnls_fit_agg", "nnls_fit_agg",
                 "anofox_stats_bls_fit_predict_agg", "bls_fit_predict_agg"):
        assert name in pkg.SQL_FUNCTIONS


def test_abi_layout():
    abi = import_pkg("_abi")
    o, r = abi.AnofoxBlsOptions, abi.AnofoxBlsFitResultCore
    assert C.sizeof(o) == 56 and C.sizeof(abi.AnofoxHipBlsBatchOptions) == 56
    assert [getattr(o, f).offset for f, _ in o._fields_] == [0, 8, 16, 24, 32, 40, 48]
    assert C.sizeof(r) == 80
    assert [getattr(r, f).offset for f, _ in r._fields_] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 72]
    # the header declares the same fields in the same order, and every new symbol
    with open(os.path.join(ROOT, "include", "anofox_stats_hip.h")) as f:
        h = f.read()
    body = re.search(r"typedef struct \{([^}]*)\} AnofoxBlsOptions;", h).group(1)
    assert re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == [f for f, _ in o._fields_]
    body = re.search(r"typedef struct \{([^}]*)\} AnofoxBlsFitResultCore;", h).group(1)
    assert re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == [f for f, _ in r._fields_]
    for sym in ("anofox_bls_fit", "anofox_nnls_fit", "anofox_free_bls_result", "anofox_hip_bls_record_len",
                "anofox_hip_bls_fit_batch_device", "anofox_hip_bls_fit_batch_host", "anofox_hip_bls_fit_predict_batch_device",
                "anofox_hip_bls_fit_predict_batch_host"):
        assert sym in abi.SYMBOLS and re.search(r"\b" + sym + r"\(", h), sym
    lib = abi.load()
    assert lib.anofox_hip_bls_record_len(5) == 21
    lib.anofox_free_bls_result(None)           # NULL-safe


# ---- the DuckDB glue (duckdb_shim/bls_family_hip.cpp) through its test driver: binding needs no device ----
GLUE = os.path.join(ROOT, "anofox-statistics_amd", "duckdb_shim", "libanofox_bls_family_capi.so")
FIT_NAMES = ["anofox_stats_bls_fit_agg", "bls_fit_agg", "anofox_stats_nnls_fit_agg", "nnls_fit_agg"]
PREDICT_NAMES = ["anofox_stats_bls_fit_predict_agg", "bls_fit_predict_agg"]


def glue_lib():
    import_pkg()
    lib = C.CDLL(GLUE)
    lib.blsf_open.restype = C.c_void_p
    lib.blsf_open.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_char_p]
    lib.blsp_open.restype = C.c_void_p
    lib.blsp_open.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_char_p]
    for pre in ("blsf", "blsp"):
        getattr(lib, pre + "_close").argtypes = [C.c_void_p]
        getattr(lib, pre + "_registered").argtypes = [C.c_void_p, C.c_char_p]
        getattr(lib, pre + "_overloads").argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int)]
    lib.blsf_result_fields.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    lib.blsp_result_fields.argtypes = [C.c_void_p]
    return lib


def test_glue_names_overloads_and_result_types_bind():
    lib = glue_lib()
    msg = C.create_string_buffer(512)
    for fn in FIT_NAMES:
        for spec, as_map in ((None, 0), ("lower=-1;upper=2", 1), ("fit_intercept=true;max_iter=5", 0)):
            q = lib.blsf_open(fn.encode(), None if spec is None else spec.encode(), as_map, msg)
            assert q, (fn, spec, msg.value.decode())
            kinds = (C.c_int * 16)()
            # STRUCT(coefficients LIST(DOUBLE), intercept, ssr, r_squared DOUBLE, three BIGINT, two LIST(BOOLEAN))
            assert lib.blsf_result_fields(q, kinds) == 9 and list(kinds[:9]) == [2, 0, 0, 0, 1, 1, 1, 3, 3]
            ov = (C.c_int * 8)()
            assert sorted(ov[:lib.blsf_overloads(q, fn.encode(), ov)]) == [2, 3]
            for name in FIT_NAMES:
                assert lib.blsf_registered(q, name.encode()) == 1
            lib.blsf_close(q)
    for fn in PREDICT_NAMES:
        for spec, split in ((None, 0), ("lower_bound=0", 0), (None, 1), ("upper=1;confidence=0.9", 1)):
            q = lib.blsp_open(fn.encode(), None if spec is None else spec.encode(), 0, split, msg)
            assert q, (fn, spec, split, msg.value.decode())
            assert lib.blsp_result_fields(q) == 5            # LIST(STRUCT(y, yhat, yhat_lower, yhat_upper, is_training))
            ov = (C.c_int * 8)()
            assert sorted(ov[:lib.blsp_overloads(q, fn.encode(), ov)]) == [2, 3, 3, 4]
            for name in PREDICT_NAMES:
                assert lib.blsp_registered(q, name.encode()) == 1
            lib.blsp_close(q)
    assert not lib.blsf_open(b"bls_fit_predict_agg", None, 0, msg)      # not a fit aggregate


def test_glue_bad_options_fail_at_bind():
    lib = glue_lib()
    msg = C.create_string_buffer(512)
    for spec, text in (("null_policy=bogus", "Invalid null_policy: 'bogus'. Valid values are 'drop', 'drop_y_zero_x'"),
                       ("max_iterations=-1", "out of range for UINTEGER")):
        assert not lib.blsp_open(b"bls_fit_predict_agg", spec.encode(), 0, 0, msg)
        assert text in msg.value.decode(), msg.value.decode()
    assert not lib.blsf_open(b"nnls_fit_agg", b"max_iter=-3", 0, msg) and "UINTEGER" in msg.value.decode()


def test_glue_under_sanitizers_on_a_mock_abi(tmp_path):
    """bls_family_hip.cpp + its driver with a mock of the C ABI under ASan / UBSan, -Wall -Wextra -Werror: threaded Update,
    Combine, Finalize by vectors, NULL results, Destroy (tests/tools/bls_glue_sanitize.cpp)."""
    import subprocess
    shim = os.path.join(ROOT, "anofox-statistics_amd", "duckdb_shim")
    tools = os.path.join(ROOT, "tests", "tools")
    exe = str(tmp_path / "bls_glue_sanitize")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", "-I" + os.path.join(tools, "duckdb_stub"),
                        "-I" + os.path.join(ROOT, "include"), "-I" + shim, os.path.join(tools, "bls_glue_sanitize.cpp"),
                        os.path.join(tools, "bls_family_capi.cpp"), os.path.join(shim, "bls_family_hip.cpp"), "-o", exe, "-lpthread"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "all scenarios passed" in r.stdout, r.stdout + r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
