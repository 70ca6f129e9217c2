"""CPU tier of the normality tests, second half: csrc/normality_tests.h in its host build (tests/tools/normality_test_host.cpp, a
program of its own compiled under ASan / UBSan, never loaded into python) held to tests/normality_test_restate.py over its case
set on both size paths; then the ABI: the header compiles as C, the struct layouts (the reference's), the exported symbols, and
the argument errors that are answered before any GPU work."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import normality_test_restate as R
from conftest import ROOT, import_pkg

BATCH_SYMBOLS = ("anofox_hip_normality_test_record_len", "anofox_hip_normality_test_batch_device", "anofox_hip_normality_test_batch_host",
                 "anofox_hip_normality_test_hooks")
SCALAR_SYMBOLS = ("anofox_shapiro_wilk", "anofox_dagostino_k2", "anofox_jarque_bera")
_DP = C.POINTER(C.c_double)
_IP = C.POINTER(C.c_int64)
NAN = float("nan")


# ---- the host build against the restatement ----
@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """tests/tools/normality_test_host.cpp as a program of its own, under ASan / UBSan.  Where a process-wide LD_PRELOAD is set a
    sanitizer's runtime could not be the first one loaded, so there the same program is built without them and the cases still
    run."""
    exe = str(tmp_path_factory.mktemp("normality_test") / "normality_test_host")
    sanitize = [] if os.environ.get("LD_PRELOAD") else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *sanitize, "-fno-omit-frame-pointer", "-g", "-O1",
                        os.path.join(ROOT, "tests", "tools", "normality_test_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def host_normality_test(host_exe):
    def run(test, call, cap=1462):
        head = np.array([test, cap, len(call["off"]) - 1, len(call["v"])], np.float64)
        out = subprocess.run([host_exe], input=np.concatenate([head, np.asarray(call["off"], np.float64), call["v"]]).tobytes(),
                             capture_output=True)
        err = out.stderr.decode()
        assert out.returncode == 0, out.stdout.decode()[-2000:] + err[-4000:]
        assert "ERROR" not in err and "runtime error" not in err, err[-4000:]
        return np.array([float(t) for t in out.stdout.decode().split()]).reshape(-1, 8)
    return run


@pytest.mark.parametrize("content", R.CONTENTS)
@pytest.mark.parametrize("name", list(R.TESTS))
def test_both_paths_against_the_restatement(host_normality_test, name, content):
    """The case set (every size of SIZES_CPU in one call) and the GPU tier's sizes, at the default cap and at a cap of 128."""
    test = R.TESTS[name]
    call = R.make_call(content, R.SIZES_CPU + R.SIZES_GPU)
    ref = R.reference(test, call)
    small, large = host_normality_test(test, call), host_normality_test(test, call, cap=128)
    print(name, content, {k: "%.2e" % v for k, v in R.check_records(test, small, ref).items()})
    assert small.tobytes() == large.tobytes()      # the lead wavefront runs the same code on either path
    assert np.any(ref[:, 7] == 0) != (content == "all_equal" and test != R.SHAPIRO_WILK)


def test_row_limit_of_shapiro_wilk(host_normality_test):
    rng = np.random.default_rng(3)
    call = dict(off=np.array([0, 5001, 5001 + 5003], np.int64), v=rng.standard_normal(5001 + 5003))
    call["v"][5001 + np.array([5, 77, 4000])] = NAN                # the second group: 5003 rows, 5000 of them valid
    for test in R.TESTS.values():
        got, ref = host_normality_test(test, call), R.reference(test, call)
        R.check_records(test, got, ref)
        assert list(got[:, 6]) == [5001.0, 5000.0]
        assert list(got[:, 7]) == ([1.0, 0.0] if test == R.SHAPIRO_WILK else [0.0, 0.0])


def test_infinities_hand_values_and_tables(host_normality_test):
    one = lambda v: dict(off=np.array([0, len(v)], np.int64), v=np.asarray(v, np.float64))   # noqa: E731
    for test in R.TESTS.values():
        call = one([1.0, np.inf, 2.0, 3.0, -1.0, 0.5, 7.0, 2.5, -np.inf])
        R.check_records(test, host_normality_test(test, call), R.reference(test, call))
    rec = host_normality_test(R.SHAPIRO_WILK, one([1.0, 2.0, 4.0]))[0]
    closed = 6.0 / np.pi * (np.arcsin(np.sqrt(27.0 / 28.0)) - np.arcsin(np.sqrt(0.75)))
    assert abs(rec[0] - 27.0 / 28.0) <= 1e-14 and abs(rec[1] - closed) <= 1e-14
    rec = host_normality_test(R.SHAPIRO_WILK, one([3.0, 1.0, 2.0]))[0]
    assert abs(rec[0] - 1.0) <= 1e-14 and abs(rec[1] - 1.0) <= 1e-14
    rec = host_normality_test(R.JARQUE_BERA, one([0.0, 1.0, 2.0]))[0]
    assert abs(rec[0] - 0.28125) <= 1e-14 and abs(rec[1] - np.exp(-0.140625)) <= 1e-14
    tables = R.load_tables(os.path.join(ROOT, "tests", "golden", "normality_tests"))

    def by_host(name, _, v):
        recs = [host_normality_test(R.TESTS[name], one(v), cap=cap)[0] for cap in (1462, 3)]
        assert np.array_equal(recs[0], recs[1], equal_nan=True)
        return R.as_row(recs[0])
    R.check_known_answers(tables, by_host)


# ---- the ABI ----
def test_symbols_present():
    abi = import_pkg("_abi")
    lib = abi.load()
    for name in BATCH_SYMBOLS + SCALAR_SYMBOLS:
        assert name in abi.SYMBOLS and getattr(lib, name) is not None
    assert lib.anofox_hip_normality_test_record_len() == 8
    pkg = import_pkg()
    for name in ("shapiro_wilk", "dagostino_k2", "jarque_bera"):
        for full in (name, name + "_agg"):
            assert pkg.SQL_FUNCTIONS[full] is pkg.SQL_FUNCTIONS["anofox_stats_" + full] is getattr(pkg, full) and full in pkg.__all__
    for name in ("normality_test_batch_host", "normality_test_batch_device", "normality_test_hooks"):
        assert callable(getattr(pkg, name)) and name in pkg.__all__
    assert callable(pkg.Context.normality_test_batch_host) and callable(pkg.Context.normality_test_batch_device)


def test_header_compiles_as_c_and_layouts_match_reference_abi():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "anofox_stats_hip.h"
#define O(T, f) printf("%zu ", offsetof(T, f))
int main(void) {
  printf("%zu %zu %zu\n", sizeof(AnofoxTestResult), sizeof(AnofoxJarqueBeraResult), sizeof(AnofoxHipNormalityTestBatchOptions));
  O(AnofoxJarqueBeraResult, statistic); O(AnofoxJarqueBeraResult, p_value); O(AnofoxJarqueBeraResult, skewness);
  O(AnofoxJarqueBeraResult, kurtosis); O(AnofoxJarqueBeraResult, n);
  printf("\n");
  O(AnofoxTestResult, statistic); O(AnofoxTestResult, p_value); O(AnofoxTestResult, df); O(AnofoxTestResult, effect_size);
  O(AnofoxTestResult, ci_lower); O(AnofoxTestResult, ci_upper); O(AnofoxTestResult, confidence_level); O(AnofoxTestResult, n);
  O(AnofoxTestResult, n1); O(AnofoxTestResult, n2); O(AnofoxTestResult, alternative); O(AnofoxTestResult, method);
  printf("\n");
  O(AnofoxHipNormalityTestBatchOptions, test);
  printf("\n");
  return 0;
}
'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.check_output([exe]).decode().split("\n")
    # the layouts of src/include/anofox_stats_ffi.h:1555-1583 and 621-632 under gcc, x86-64 SysV
    assert [int(v) for v in out[0].split()] == [96, 40, 8]
    assert [int(v) for v in out[1].split()] == [0, 8, 16, 24, 32]
    assert [int(v) for v in out[2].split()] == list(range(0, 96, 8))
    assert [int(v) for v in out[3].split()] == [0]
    abi = import_pkg("_abi")
    types = (abi.AnofoxTestResult, abi.AnofoxJarqueBeraResult, abi.AnofoxHipNormalityTestBatchOptions)
    assert [C.sizeof(t) for t in types] == [96, 40, 8]
    assert [getattr(abi.AnofoxJarqueBeraResult, f).offset for f, _ in abi.AnofoxJarqueBeraResult._fields_] == [0, 8, 16, 24, 32]


def _batch(lib, abi, n_groups=1, n_rows=4, off=(0, 4), v=True, records=True, offsets=True, test=0):
    o = np.array(off, np.int64)
    vv, rec = np.ones(64), np.zeros(64)
    err = abi.AnofoxError()
    p = lambda a, on: a.ctypes.data_as(_DP) if on else None   # noqa: E731
    ok = lib.anofox_hip_normality_test_batch_host(None, n_groups, n_rows, o.ctypes.data_as(_IP) if offsets else None, p(vv, v),
                                                  abi.AnofoxHipNormalityTestBatchOptions(test, 0), p(rec, records), C.byref(err))
    return ok, err.code, err.text()


@pytest.mark.parametrize("kw, text", [
    (dict(v=False), "normality test: row_offsets, v or records is NULL"), (dict(records=False), "normality test: row_offsets, v or records is NULL"),
    (dict(offsets=False), "normality test: row_offsets, v or records is NULL"),
    (dict(off=(0, 3, 2), n_groups=2), "non-decreasing"), (dict(off=(0, 5)), "non-decreasing"), (dict(off=(-1, 4)), "non-decreasing"),
    (dict(n_groups=-1), "negative"), (dict(n_rows=-1), "negative"),
    (dict(test=3), "normality test: unknown test"), (dict(test=-1), "normality test: unknown test")])
def test_batch_argument_errors_come_before_any_device(kw, text):
    abi = import_pkg("_abi")
    ok, code, msg = _batch(abi.load(), abi, **kw)
    assert not ok and code == 1 and text in msg, msg


def test_device_form_checks_its_arguments_first_and_an_empty_call_succeeds():
    abi = import_pkg("_abi")
    lib, err = abi.load(), abi.AnofoxError()
    good, bad = abi.AnofoxHipNormalityTestBatchOptions(0, 0), abi.AnofoxHipNormalityTestBatchOptions(9, 0)
    assert not lib.anofox_hip_normality_test_batch_device(None, 1, 4, None, None, good, None, C.byref(err)) and err.code == 1
    assert not lib.anofox_hip_normality_test_batch_device(None, 1, 4, 8, 8, bad, 8, C.byref(err)) and "normality test: unknown test" in err.text()
    assert not lib.anofox_hip_normality_test_batch_device(None, 1, 4, 8, 8, good, 8, C.byref(err)) and "context is NULL" in err.text()
    assert lib.anofox_hip_normality_test_batch_host(None, 0, 0, None, None, good, None, C.byref(err)) and err.code == 0   # nothing to do
    lib.anofox_hip_normality_test_hooks(128)
    lib.anofox_hip_normality_test_hooks(0)


def _scalar(abi, symbol, values, result):
    res, err = result(), abi.AnofoxError()
    C.memset(C.byref(res), 0xAB, C.sizeof(res))
    a = np.asarray(values, np.float64)
    ok = getattr(abi.load(), symbol)(abi.AnofoxDataArray(a.ctypes.data_as(_DP), None, len(a)), C.byref(res), C.byref(err))
    return ok, res, err


def test_scalar_failures_leave_the_result_zeroed():
    """The reference's texts and codes, answered from the count of the valid rows alone: no device is touched."""
    abi = import_pkg("_abi")
    T, J = abi.AnofoxTestResult, abi.AnofoxJarqueBeraResult
    cases = [("anofox_shapiro_wilk", [1.0, 2.0], T, 6, "Shapiro-Wilk test requires at least 3 observations"),
             ("anofox_shapiro_wilk", [1.0, NAN, 2.0, NAN], T, 6, "Shapiro-Wilk test requires at least 3 observations"),
             ("anofox_shapiro_wilk", np.arange(5001.0), T, 1, "Shapiro-Wilk test is limited to n <= 5000"),
             ("anofox_dagostino_k2", np.arange(7.0), T, 6, "D'Agostino K-squared test requires at least 8 observations"),
             ("anofox_dagostino_k2", [], T, 6, "D'Agostino K-squared test requires at least 8 observations"),
             ("anofox_jarque_bera", [1.0, 2.0, NAN], J, 6, "Jarque-Bera test requires at least 3 observations")]
    for symbol, values, result, code, text in cases:
        ok, res, err = _scalar(abi, symbol, values, result)
        assert not ok and err.code == code and text in err.text(), err.text()
        assert bytes(res) == bytes(C.sizeof(res))          # every field 0, the pointer NULL: nothing to free
        if result is T:
            abi.load().anofox_free_test_result(C.byref(res))   # harmless
    err, empty = abi.AnofoxError(), abi.AnofoxDataArray(None, None, 0)
    for symbol in SCALAR_SYMBOLS:
        assert not getattr(abi.load(), symbol)(empty, None, C.byref(err)) and err.code == 1 and "out_result is NULL" in err.text()


def test_python_refuses_bad_input_before_any_device():
    pkg = import_pkg()
    with pytest.raises(pkg.InvalidInputException, match="Shapiro-Wilk test requires at least 3 observations"):
        pkg.shapiro_wilk([1.0, 2.0])
    with pytest.raises(pkg.InvalidInputException, match="at least 8 observations"):
        pkg.dagostino_k2([1.0, 2.0, 3.0])
    with pytest.raises(pkg.InvalidInputException, match="Jarque-Bera test requires at least 3 observations"):
        pkg.jarque_bera([1.0])
    with pytest.raises(pkg.InvalidInputException, match="same number of rows"):
        pkg.shapiro_wilk_agg(["a", "a"], [1.0, 2.0, 3.0])
    with pytest.raises(pkg.AnofoxStatsError, match="unknown test"):
        pkg.normality_test_batch_host(np.array([0, 3], np.int64), np.arange(3.0), 7)
