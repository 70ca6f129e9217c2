"""CPU tier of the categorical tests, second half: csrc/categorical_tests.h in its host build (tests/tools/categorical_test_host.cpp,
a program of its own compiled under ASan / UBSan, never loaded into python) held to tests/categorical_test_restate.py over its case
set on both size paths; then the ABI: the header compiles as C, the struct layouts (the reference's), the exported symbols, the
argument errors that are answered before any GPU work, and the table- and cell-taking scalars, which touch no device."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import categorical_test_restate as R
from conftest import ROOT, import_pkg
from test_categorical_test_restate_cpu import restated_aggregate

BATCH_SYMBOLS = ("anofox_hip_categorical_test_record_len", "anofox_hip_categorical_test_batch_device",
                 "anofox_hip_categorical_test_batch_host", "anofox_hip_categorical_test_hooks")
SCALAR_SYMBOLS = ("anofox_chisq_test", "anofox_free_chisq_result", "anofox_g_test", "anofox_cramers_v", "anofox_contingency_coef",
                  "anofox_fisher_exact", "anofox_mcnemar_test", "anofox_phi_coefficient")
_DP = C.POINTER(C.c_double)
_IP = C.POINTER(C.c_int64)
_I32P = C.POINTER(C.c_int32)
NAN = float("nan")


# ---- the host build against the restatement ----
@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """tests/tools/categorical_test_host.cpp as a program of its own, under ASan / UBSan.  Where a process-wide LD_PRELOAD is set a
    sanitizer's runtime could not be the first one loaded, so there the same program is built without them and the cases still
    run."""
    exe = str(tmp_path_factory.mktemp("categorical_test") / "categorical_test_host")
    sanitize = [] if os.environ.get("LD_PRELOAD") else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *sanitize, "-fno-omit-frame-pointer", "-g", "-O1",
                        os.path.join(ROOT, "tests", "tools", "categorical_test_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def host_categorical_test(host_exe):
    def run(test, call, cap=1462):
        o = R.options(**call.get("opts", {}))
        level = NAN if o["confidence_level"] is None else o["confidence_level"]
        head = np.array([test, o["alternative"], o["correction"], o["exact"], level, cap, len(call["off"]) - 1, len(call["a"])], np.float64)
        data = np.concatenate([head, np.asarray(call["off"], np.float64), np.asarray(call["a"], np.float64), np.asarray(call["b"], np.float64)])
        out = subprocess.run([host_exe], input=data.tobytes(), capture_output=True)
        err = out.stderr.decode()
        assert out.returncode == 0, out.stdout.decode()[-2000:] + err[-4000:]
        assert "ERROR" not in err and "runtime error" not in err, err[-4000:]
        return np.array([float(t) for t in out.stdout.decode().split()]).reshape(-1, 12)
    return run


def _both_caps(run, test, call):
    ref = R.reference(test, call)
    small, large = run(test, call), run(test, call, cap=128)
    assert small.tobytes() == large.tobytes()      # the lead wavefront runs the same code on either path
    return R.check_records(test, small, ref)


@pytest.mark.parametrize("content", R.CONTENTS)
@pytest.mark.parametrize("name", list(R.TESTS))
def test_both_paths_against_the_restatement(host_categorical_test, name, content):
    """The case set (every size of SIZES in one call) at the default cap and at a cap of 128."""
    test = R.TESTS[name]
    errs = _both_caps(host_categorical_test, test, R.make_call(content))
    if test == R.CHI_SQUARE:
        errs.update(_both_caps(host_categorical_test, test, R.make_call(content, opts=dict(correction=True))))
    print(name, content, {k: "%.2e" % v for k, v in errs.items()})


@pytest.mark.parametrize("alternative", (R.TWO_SIDED, R.LESS, R.GREATER))
def test_fisher_tables(host_categorical_test, alternative):
    for level in (0.95, 0.9, None):
        call = R.cells_call(R.FISHER_TABLES, dict(alternative=alternative, confidence_level=level))
        errs = R.check_records(R.FISHER_EXACT, host_categorical_test(R.FISHER_EXACT, call), R.reference(R.FISHER_EXACT, call))
        print("fisher", alternative, level, {k: "%.2e" % v for k, v in errs.items()})


def test_mcnemar_tables(host_categorical_test):
    for opts in (dict(correction=True), dict(correction=False), dict(exact=True)):
        call = R.cells_call(R.MCNEMAR_TABLES, opts)
        call["a"], call["b"] = call["a"] * 7, call["b"] * -3          # every label but 0 is "1"
        got = host_categorical_test(R.MCNEMAR, call)
        R.check_records(R.MCNEMAR, got, R.reference(R.MCNEMAR, call))
        assert np.isnan(got[0, 0]) and np.isnan(got[0, 1]) and got[0, 11] == 0       # b + c = 0


def test_the_sql_tables_by_the_host_build(host_categorical_test):
    fixtures = R.load_tables(os.path.join(ROOT, "tests", "golden", "categorical_tests"))

    def by_host(function, a, b):
        test = {"g_test": R.G_TEST, "fisher_exact": R.FISHER_EXACT, "mcnemar": R.MCNEMAR}.get(function, R.CHI_SQUARE)
        call = dict(off=np.array([0, len(a)], np.int64), a=a, b=b, opts=dict(correction=function == "mcnemar"))
        R.check_records(test, host_categorical_test(test, call), R.reference(test, call))
        return restated_aggregate(function, a, b)
    R.check_known_answers(fixtures, by_host)


# ---- the ABI ----
def test_symbols_present():
    abi = import_pkg("_abi")
    lib = abi.load()
    for name in BATCH_SYMBOLS + SCALAR_SYMBOLS:
        assert name in abi.SYMBOLS and getattr(lib, name) is not None
    assert lib.anofox_hip_categorical_test_record_len() == 12
    pkg = import_pkg()
    for full in ("chisq_test", "g_test", "fisher_exact", "mcnemar_test", "cramers_v", "phi_coefficient", "contingency_coef", "chisq_test_agg",
                 "g_test_agg", "fisher_exact_agg", "mcnemar_agg", "cramers_v_agg", "phi_coefficient_agg", "contingency_coef_agg"):
        assert pkg.SQL_FUNCTIONS[full] is pkg.SQL_FUNCTIONS["anofox_stats_" + full] is getattr(pkg, full) and full in pkg.__all__
    for name in ("categorical_test_batch_host", "categorical_test_batch_device", "categorical_test_hooks", "parse_categorical_test_options"):
        assert callable(getattr(pkg, name)) and name in pkg.__all__
    assert callable(pkg.Context.categorical_test_batch_host) and callable(pkg.Context.categorical_test_batch_device)


def test_header_compiles_as_c_and_layouts_match_reference_abi():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "anofox_stats_hip.h"
#define O(T, f) printf("%zu ", offsetof(T, f))
int main(void) {
  printf("%zu %zu %zu %zu\n", sizeof(AnofoxChiSquareResult), sizeof(AnofoxChiSquareOptions), sizeof(AnofoxFisherExactOptions),
         sizeof(AnofoxHipCategoricalTestBatchOptions));
  O(AnofoxChiSquareResult, statistic); O(AnofoxChiSquareResult, p_value); O(AnofoxChiSquareResult, df); O(AnofoxChiSquareResult, method);
  printf("\n");
  O(AnofoxFisherExactOptions, alternative); O(AnofoxFisherExactOptions, confidence_level);
  printf("\n");
  O(AnofoxHipCategoricalTestBatchOptions, test); O(AnofoxHipCategoricalTestBatchOptions, alternative);
  O(AnofoxHipCategoricalTestBatchOptions, correction); O(AnofoxHipCategoricalTestBatchOptions, exact);
  O(AnofoxHipCategoricalTestBatchOptions, confidence_level);
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
    # the layouts of src/include/anofox_stats_ffi.h:1634-1643, 1743-1746 and 1751-1756 under gcc, x86-64 SysV
    assert [int(v) for v in out[0].split()] == [32, 1, 16, 24]
    assert [int(v) for v in out[1].split()] == [0, 8, 16, 24]
    assert [int(v) for v in out[2].split()] == [0, 8]
    assert [int(v) for v in out[3].split()] == [0, 4, 8, 12, 16]
    abi = import_pkg("_abi")
    types = (abi.AnofoxChiSquareResult, abi.AnofoxChiSquareOptions, abi.AnofoxFisherExactOptions, abi.AnofoxHipCategoricalTestBatchOptions)
    assert [C.sizeof(t) for t in types] == [32, 1, 16, 24]
    assert [getattr(abi.AnofoxChiSquareResult, f).offset for f, _ in abi.AnofoxChiSquareResult._fields_] == [0, 8, 16, 24]
    assert [getattr(abi.AnofoxHipCategoricalTestBatchOptions, f).offset for f, _ in abi.AnofoxHipCategoricalTestBatchOptions._fields_] == [0, 4, 8, 12, 16]


def _batch(lib, abi, n_groups=1, n_rows=4, off=(0, 4), a=True, b=True, records=True, offsets=True, test=0, alternative=0, level=0.95):
    o = np.array(off, np.int64)
    aa, bb, rec = np.ones(64, np.int32), np.ones(64, np.int32), np.zeros(64)
    err = abi.AnofoxError()
    ok = lib.anofox_hip_categorical_test_batch_host(None, n_groups, n_rows, o.ctypes.data_as(_IP) if offsets else None,
                                                    aa.ctypes.data_as(_I32P) if a else None, bb.ctypes.data_as(_I32P) if b else None,
                                                    abi.AnofoxHipCategoricalTestBatchOptions(test, alternative, 0, 0, level),
                                                    rec.ctypes.data_as(_DP) if records else None, C.byref(err))
    return ok, err.code, err.text()


@pytest.mark.parametrize("kw, text", [
    (dict(a=False), "categorical test: row_offsets, a, b or records is NULL"), (dict(b=False), "categorical test: row_offsets, a, b or records is NULL"),
    (dict(records=False), "categorical test: row_offsets, a, b or records is NULL"),
    (dict(offsets=False), "categorical test: row_offsets, a, b or records is NULL"),
    (dict(off=(0, 3, 2), n_groups=2), "non-decreasing"), (dict(off=(0, 5)), "non-decreasing"), (dict(off=(-1, 4)), "non-decreasing"),
    (dict(n_groups=-1), "categorical test: negative"), (dict(n_rows=-1), "categorical test: negative"),
    (dict(test=4), "categorical test: unknown test"), (dict(test=-1), "categorical test: unknown test"),
    (dict(alternative=3), "categorical test: unknown alternative"), (dict(alternative=-1), "categorical test: unknown alternative"),
    (dict(level=0.0), "categorical test: confidence_level"), (dict(level=1.0), "categorical test: confidence_level"),
    (dict(level=float("inf")), "categorical test: confidence_level")])
def test_batch_argument_errors_come_before_any_device(kw, text):
    abi = import_pkg("_abi")
    ok, code, msg = _batch(abi.load(), abi, **kw)
    assert not ok and code == 1 and text in msg, msg


def test_device_form_checks_its_arguments_first_and_an_empty_call_succeeds():
    abi = import_pkg("_abi")
    lib, err = abi.load(), abi.AnofoxError()
    good, bad = abi.AnofoxHipCategoricalTestBatchOptions(0, 0, 0, 0, NAN), abi.AnofoxHipCategoricalTestBatchOptions(9, 0, 0, 0, 0.95)
    assert not lib.anofox_hip_categorical_test_batch_device(None, 1, 4, None, None, None, good, None, C.byref(err)) and err.code == 1
    assert not lib.anofox_hip_categorical_test_batch_device(None, 1, 4, 8, 8, 8, bad, 8, C.byref(err)) and "categorical test: unknown test" in err.text()
    assert not lib.anofox_hip_categorical_test_batch_device(None, 1, 4, 8, 8, 8, good, 8, C.byref(err)) and "context is NULL" in err.text()
    assert lib.anofox_hip_categorical_test_batch_host(None, 0, 0, None, None, None, good, None, C.byref(err)) and err.code == 0   # nothing to do
    lib.anofox_hip_categorical_test_hooks(128)
    lib.anofox_hip_categorical_test_hooks(0)


def test_table_and_cell_scalars_touch_no_device():
    """The scalars that take counts against the restatement, on hand tables and on the tables of the reference's SQL tests."""
    pkg = import_pkg()
    t = np.array([[10, 20], [30, 40]])
    g = pkg.g_test(t)
    ref = R.table_record(R.G_TEST, t, False)
    assert abs(g["statistic"] - ref[0]) <= 1e-12 and abs(g["p_value"] - ref[1]) <= 1e-12 and g["df"] == 1 and g["method"].startswith("G-test")
    ref = R.table_record(R.CHI_SQUARE, t, False)
    assert abs(pkg.cramers_v(t) - ref[3]) <= 1e-14 and abs(pkg.contingency_coef(t) - ref[9]) <= 1e-14
    assert abs(pkg.phi_coefficient(10, 20, 30, 40) - ref[10]) <= 1e-14 and ref[10] < 0
    ragged = [[3, 0, 4], [0, 0], [5, 0, 1, 0]]                      # an empty row and two empty columns are dropped; a short row's cells are 0
    ref = R.table_record(R.CHI_SQUARE, np.array([[3, 4], [5, 1]]), False)
    assert abs(pkg.cramers_v(ragged) - ref[3]) <= 1e-14
    for cells in R.FISHER_TABLES:
        for alt, name in ((R.TWO_SIDED, "two_sided"), (R.LESS, "less"), (R.GREATER, "greater")):
            d = pkg.fisher_exact(*cells, options=dict(alternative=name, confidence_level=0.9))
            got = np.array([d["statistic"], d["p_value"], d["df"], d["effect_size"], d["ci_lower"], d["ci_upper"], d["n"], 2, 2, NAN, NAN, 0])
            R.check_records(R.FISHER_EXACT, got, R.fisher_record(cells, alt, 0.9))
            assert d["method"] == "Fisher's exact test" and d["alternative"] == alt and d["confidence_level"] == 0.9 and (d["n1"], d["n2"]) == (0, 0)
    for cells in R.MCNEMAR_TABLES[1:]:
        for opts in (dict(correction=True), dict(correction=False), dict(exact=True)):
            d = pkg.mcnemar_test(*cells, options=opts)
            ref = R.mcnemar_record(cells, opts.get("correction", True), opts.get("exact", False))
            assert abs(d["p_value"] - ref[1]) <= 1e-9 * ref[1] and d["df"] == (0 if opts.get("exact") else 1) and "McNemar" in d["method"]
            assert np.isnan(d["statistic"]) if opts.get("exact") else abs(d["statistic"] - ref[0]) <= 1e-12 * max(1.0, ref[0])
    fixtures = R.load_tables(os.path.join(ROOT, "tests", "golden", "categorical_tests"))

    def by_scalar(function, a, b):
        if function in ("g_test", "cramers_v", "contingency_coef"):
            got = getattr(pkg, function)(R.dense_table(a, b))
        elif function == "phi_coefficient":
            got = pkg.phi_coefficient(*R.dense_table(a, b).ravel())
        elif function == "fisher_exact":
            d = pkg.fisher_exact(*R.cells_of(R.FISHER_EXACT, a, b))
            got = dict(statistic=d["statistic"], p_value=d["p_value"], odds_ratio=d["statistic"], conditional_odds_ratio=d["effect_size"],
                       ci_lower=d["ci_lower"], ci_upper=d["ci_upper"], n=d["n"])
        elif function == "mcnemar":
            got = pkg.mcnemar_test(*R.cells_of(R.MCNEMAR, a, b))
        else:
            return restated_aggregate(function, a, b)       # anofox_chisq_test runs on the device: tests/test_gpu_categorical_tests.py
        ref = restated_aggregate(function, a, b)
        for key in (ref if isinstance(ref, dict) else ()):
            assert abs(got[key] - ref[key]) <= 1e-9 * max(1.0, abs(ref[key])), (function, key, got, ref)
        return got
    R.check_known_answers(fixtures, by_scalar)


def test_scalar_failures_leave_nothing_to_free():
    abi = import_pkg("_abi")
    lib, err = abi.load(), abi.AnofoxError()
    res = abi.AnofoxChiSquareResult()
    C.memset(C.byref(res), 0xAB, C.sizeof(res))
    table, lengths = (C.c_size_t * 4)(5, 0, 7, 0), (C.c_size_t * 2)(2, 2)
    assert not lib.anofox_g_test(table, lengths, 2, C.byref(res), C.byref(err)) and err.code == 1 and "at least 2" in err.text()
    assert bytes(res) == bytes(C.sizeof(res))
    lib.anofox_free_chisq_result(C.byref(res))      # harmless
    assert not lib.anofox_g_test(None, lengths, 2, C.byref(res), C.byref(err)) and "Invalid table data" in err.text()
    assert not lib.anofox_g_test(table, lengths, 2, None, C.byref(err)) and "out_result is NULL" in err.text()
    out = C.c_double(7.0)
    assert not lib.anofox_cramers_v(table, lengths, 0, C.byref(out), C.byref(err)) and "Invalid table data" in err.text()
    assert not lib.anofox_phi_coefficient(0, 0, 3, 4, C.byref(out), C.byref(err)) and err.code == 1
    fisher = abi.AnofoxTestResult()
    C.memset(C.byref(fisher), 0xAB, C.sizeof(fisher))
    assert not lib.anofox_fisher_exact(0, 0, 0, 0, abi.AnofoxFisherExactOptions(0, 0.95), C.byref(fisher), C.byref(err)) and err.code == 6
    assert bytes(fisher) == bytes(C.sizeof(fisher))
    assert not lib.anofox_fisher_exact(1, 2, 3, 4, abi.AnofoxFisherExactOptions(0, 1.5), C.byref(fisher), C.byref(err)) and "confidence_level" in err.text()
    assert not lib.anofox_fisher_exact(1, 2, 3, 4, abi.AnofoxFisherExactOptions(7, 0.95), C.byref(fisher), C.byref(err)) and "alternative" in err.text()
    assert not lib.anofox_mcnemar_test(0, 0, 0, 0, True, False, C.byref(res), C.byref(err)) and err.code == 6
    empty = abi.AnofoxDataArray(None, None, 0)
    assert not lib.anofox_chisq_test(empty, empty, abi.AnofoxChiSquareOptions(False), C.byref(res), C.byref(err)) and err.code == 6
    assert "No valid data pairs" in err.text() and bytes(res) == bytes(C.sizeof(res))
    assert not lib.anofox_chisq_test(empty, empty, abi.AnofoxChiSquareOptions(False), None, C.byref(err)) and "out_result is NULL" in err.text()


def test_python_options_and_refusals():
    pkg = import_pkg()
    o = pkg.parse_categorical_test_options({"Continuity_Correction": "true", "ALTERNATIVE": "Greater", "exact": 1, "confidence_level": 0.9})
    assert (o.correction, o.alternative, o.exact, o.confidence_level) == (True, 2, True, 0.9)
    d = pkg.parse_categorical_test_options(None)
    assert d.resolved_correction(0) is False and d.resolved_correction(3) is True and d.alternative == 0 and d.confidence_level == 0.95
    with pytest.raises(pkg.InvalidInputException, match="same number of rows"):
        pkg.chisq_test_agg(["a", "a"], [1, 2, 3], [1, 2, 3])
    with pytest.raises(pkg.AnofoxStatsError, match="categorical test: unknown test"):
        pkg.categorical_test_batch_host(np.array([0, 3], np.int64), np.arange(3, dtype=np.int32), np.arange(3, dtype=np.int32), 7)
    with pytest.raises(ValueError):
        pkg.categorical_test_batch_host(np.array([0, 3], np.int64), np.arange(3, dtype=np.int32), np.arange(4, dtype=np.int32), 0)
    with pytest.raises(pkg.InvalidInputException, match="Invalid table data"):
        pkg.g_test([])
