"""The DuckDB glue of the quantile family (duckdb_shim/quantile_family_hip.cpp) without a GPU: what binds — the six names, their
overloads, result types, options as MAP and as STRUCT, the bind errors — through tests/tools/quantile_family_capi.cpp, and the
glue with its driver on a mock of the C ABI under ASan / UBSan as a stand-alone program (tests/tools/quantile_glue_sanitize.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import quantile_glue_cases as G
from conftest import ROOT, import_pkg

SHIM = os.path.join(ROOT, "anofox-statistics_amd", "duckdb_shim")
TOOLS = os.path.join(ROOT, "tests", "tools")
LIB = os.path.join(SHIM, "libanofox_quantile_family_capi.so")
AGG, PATH, WINDOW = 0, 1, 2
NAMES = {AGG: ("anofox_stats_quantile_fit_predict_agg", "quantile_fit_predict_agg"),
         PATH: ("anofox_stats_quantile_path_fit_predict_agg", "quantile_path_fit_predict_agg"),
         WINDOW: ("anofox_stats_quantile_fit_predict", "quantile_fit_predict")}
TAUS_MISSING = "the quantile path needs the option 'taus': a non-empty list of quantiles"
_P = C.c_void_p


@pytest.fixture(scope="module")
def lib():
    import_pkg()
    lib = C.CDLL(LIB)
    lib.qg_open.restype = _P
    lib.qg_open.argtypes = [C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_char_p]
    lib.qg_close.argtypes = [_P]
    lib.qg_registered.argtypes = [_P, C.c_char_p]
    lib.qg_overloads.argtypes = [_P, C.c_char_p, C.POINTER(C.c_int)]
    lib.qg_result_fields.argtypes = [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    return lib


def _open(lib, kind, fn, spec=None, as_map=False, split=False, foldable=True):
    """-> (handle or None, message)"""
    msg = C.create_string_buffer(512)
    q = lib.qg_open(kind, fn.encode(), None if spec is None else spec.encode(), int(as_map), int(split), int(foldable), msg)
    return q, msg.value.decode()


def test_names_overloads_and_result_types_bind(lib):
    want_overloads = {AGG: [2, 3, 3, 4], PATH: [3, 4], WINDOW: [2, 3]}
    # (is a LIST of row structs, field kinds: 0 DOUBLE, 1 BOOLEAN)
    want_fields = {AGG: (1, [0, 0, 1]),            # LIST(STRUCT(y, yhat, is_training))
                   PATH: (1, [0, 0, 0, 1]),        # LIST(STRUCT(y, tau, yhat, is_training))
                   WINDOW: (0, [0, 0, 0])}         # STRUCT(yhat, yhat_lower, yhat_upper)
    binds = {AGG: [(None, False), ("tau=0.25", False), (None, True), ("tau=0.25;fit_intercept=false", True)],
             PATH: [("taus=[0.1,0.5,0.9]", False), ("taus=[0.1,0.5,0.9];max_iter=200", True)],
             WINDOW: [(None, False), ("tau=0.9;tol=1e-8", False)]}
    for kind, names in NAMES.items():
        for fn in names:
            for spec, split in binds[kind]:
                q, text = _open(lib, kind, fn, spec, False, split)
                assert q, (fn, spec, split, text)
                for every in sum(NAMES.values(), ()):
                    assert lib.qg_registered(q, every.encode()) == 1, every            # all six names
                ov = (C.c_int * 8)()
                assert sorted(ov[:lib.qg_overloads(q, fn.encode(), ov)]) == want_overloads[kind]
                kinds, is_list = (C.c_int * 8)(), C.c_int(-1)
                k = lib.qg_result_fields(q, kinds, C.byref(is_list))
                assert (is_list.value, list(kinds[:k])) == want_fields[kind], fn
                lib.qg_close(q)
    for kind, fn in ((PATH, "quantile_path_fit_predict_agg"), (WINDOW, "quantile_fit_predict")):
        q, text = _open(lib, kind, fn, None if kind == PATH else "tau=0.5", False, kind == WINDOW)
        assert not q and "no overload" in text             # the path needs its options; the window takes no split column


@pytest.mark.parametrize("as_map", [False, True])
def test_options_bind_as_map_and_as_struct(lib, as_map):
    for kind, fn, split, spec in ((AGG, "quantile_fit_predict_agg", False, "Tau=0.9;INTERCEPT=0;max_iter=50;tol=1e-9"),
                                  (AGG, "anofox_stats_quantile_fit_predict_agg", True, "tau=0.1;fit_intercept=1;max_iterations=7;tolerance=0.5"),
                                  (AGG, "quantile_fit_predict_agg", False, "quantile=0.9;full_output=1"),      # ignored keys
                                  (AGG, "quantile_fit_predict_agg", False, "tau=1.5"),                         # not range-checked at bind
                                  (WINDOW, "quantile_fit_predict", False, "tau=0.75;quantile=0.2"),
                                  (PATH, "quantile_path_fit_predict_agg", True, "taus=[0.9,0.1,null,1.2]"),    # NULL / out of range: kept
                                  (PATH, "anofox_stats_quantile_path_fit_predict_agg", False, "TAUS=[0.5]")):
        q, text = _open(lib, kind, fn, spec, as_map, split)
        assert q, (fn, spec, text)
        lib.qg_close(q)
    if not as_map:                                          # a STRUCT mixes a LIST with scalars; a MAP has one value type
        q, text = _open(lib, PATH, "quantile_path_fit_predict_agg", "taus=[0.25,0.75];intercept=false;max_iter=10")
        assert q, text
        lib.qg_close(q)


def test_bind_errors(lib):
    uint = "out of range for UINTEGER"
    cases = [
        (AGG, "quantile_fit_predict_agg", "max_iterations=-1", True, uint),
        (AGG, "quantile_fit_predict_agg", "max_iter=4294967296.0", True, uint),
        (WINDOW, "quantile_fit_predict", "max_iter=-3", True, uint),
        (PATH, "quantile_path_fit_predict_agg", "taus=[0.5];max_iterations=-1", True, uint),
        (AGG, "quantile_fit_predict_agg", "<scalar>", True, "Options must be a MAP or STRUCT"),
        (WINDOW, "quantile_fit_predict", "<scalar>", True, "Options must be a MAP or STRUCT"),
        (PATH, "quantile_path_fit_predict_agg", "<scalar>", True, "Options must be a MAP or STRUCT"),
        (PATH, "quantile_path_fit_predict_agg", "fit_intercept=true", True, TAUS_MISSING),
        (PATH, "quantile_path_fit_predict_agg", "taus=[]", True, TAUS_MISSING),
        (PATH, "quantile_path_fit_predict_agg", "taus=0.5", True, TAUS_MISSING),                    # a number is not a list
        (PATH, "quantile_path_fit_predict_agg", "<null>", True, TAUS_MISSING),
        (PATH, "quantile_path_fit_predict_agg", "taus=[0.1,0.9];tau=0.5", True, "the quantile path takes a list of quantiles in 'taus', not 'tau'"),
        (PATH, "quantile_path_fit_predict_agg", "Tau=0.5", True, "the quantile path takes a list of quantiles in 'taus', not 'tau'"),
        (PATH, "quantile_path_fit_predict_agg", "taus=[0.1,0.9]", False, "Options parameter must be a constant expression"),
        (PATH, "quantile_path_fit_predict_agg", "taus=[" + ",".join(["0.5"] * 65) + "]", True, "quantile path: n_taus > 64 is not built"),
    ]
    for kind, fn, spec, foldable, want in cases:
        for split in ((False, True) if kind != WINDOW else (False,)):
            q, text = _open(lib, kind, fn, spec, False, split, foldable)
            assert not q and want in text, (fn, spec, text)
    q, text = _open(lib, PATH, "quantile_path_fit_predict_agg", "taus=[" + ",".join(["0.5"] * 64) + "]")
    assert q, text                                         # 64 entries are built
    lib.qg_close(q)
    # options that are not constant: the single-tau functions keep their defaults, as the reference's bind does
    q, text = _open(lib, AGG, "quantile_fit_predict_agg", "tau=0.9", False, False, False)
    assert q, text
    lib.qg_close(q)


def test_fixed_seeds_give_every_fitted_group_a_unique_optimum():
    """The restatement alone, on the inputs of tests/test_gpu_quantile_glue.py: every group, path position and window frame that
    the row rules let through has a decided, strict certificate, so the GPU test compares every one of them with the restatement
    and leaves none out."""
    certified = 0

    def check(X, y_fit, tau, fit_intercept, n_training):
        nonlocal certified
        if G.restated_status(X, y_fit, tau, fit_intercept, n_training) != 0:
            return
        assert G.restated_fit(X, y_fit, tau, fit_intercept)[1], (tau, fit_intercept, len(y_fit))
        certified += 1

    for wide, runs in ((False, [(r[3], r[4], r[5]) for r in G.AGG_RUNS] + [(r[3], t, r[4]) for r in G.PATH_RUNS for t in G.PATH_TAUS[:3]]),
                       (True, [(False, 0.5, True)])):
        case = G.group_by_case(wide)
        for split, tau, fit_intercept in sorted(set(runs)):
            groups, _, off, y_fit, X, counts = G.group_batch(case, split)
            assert len(groups) == case["K"] - (0 if wide else 1)                 # only the one-row group is NULL by the row rules
            for i in range(len(groups)):
                check(X[off[i]:off[i + 1]], y_fit[off[i]:off[i + 1]], tau, fit_intercept, int(counts[i]))
    w = G.window_case()
    yv = np.where(w["y_null"] == 1, np.nan, w["y"])
    for _, _, tau, fit_intercept in G.WINDOW_RUNS:
        for tree in (False, True):
            for lo, hi, _ in G.window_frames(w, tree):
                n_training = int(np.isfinite(yv[lo:hi]).sum())
                if n_training >= 2:
                    check(w["X"][lo:hi], yv[lo:hi], tau, fit_intercept, n_training)
    assert certified > 400


def test_glue_under_sanitizers_on_a_mock_abi(tmp_path):
    """quantile_family_hip.cpp + its driver with a mock of the C ABI under ASan / UBSan, -Wall -Wextra -Werror, as a stand-alone
    program (tests/tools/quantile_glue_sanitize.cpp).  The child inherits the environment unchanged; a process-wide preload
    would sit in front of the sanitizer's runtime, so the test does not run under one."""
    if os.environ.get("LD_PRELOAD"):
        pytest.skip("LD_PRELOAD is set: a sanitizer build must be the first runtime a process loads")
    exe = str(tmp_path / "quantile_glue_sanitize")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", "-I" + os.path.join(TOOLS, "duckdb_stub"),
                        "-I" + os.path.join(ROOT, "include"), "-I" + SHIM, os.path.join(TOOLS, "quantile_glue_sanitize.cpp"),
                        os.path.join(TOOLS, "quantile_family_capi.cpp"), os.path.join(SHIM, "quantile_family_hip.cpp"), "-o", exe, "-lpthread"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all scenarios passed" in r.stdout, r.stdout + r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
