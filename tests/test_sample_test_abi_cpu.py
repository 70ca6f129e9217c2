"""CPU-side checks of the sample test surface: the header compiles as C, the struct layouts (the reference's ABI), the exported
symbols, the option spellings, and the argument errors that are answered before any GPU work."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT, import_pkg

BATCH_SYMBOLS = ("anofox_hip_sample_test_record_len", "anofox_hip_sample_test_batch_device", "anofox_hip_sample_test_batch_host",
                 "anofox_hip_sample_test_hooks")
SCALAR_SYMBOLS = ("anofox_t_test", "anofox_yuen_test", "anofox_brunner_munzel", "anofox_one_way_anova", "anofox_brown_forsythe",
                  "anofox_free_anova_result")
_DP = C.POINTER(C.c_double)
_IP = C.POINTER(C.c_int64)
_SP = C.POINTER(C.c_int32)
NAN = float("nan")
GOOD = (0, 0, 0, 0.0, 0.2, 0.95)


def test_symbols_present():
    abi = import_pkg("_abi")
    lib = abi.load()
    for name in BATCH_SYMBOLS + SCALAR_SYMBOLS:
        assert name in abi.SYMBOLS and getattr(lib, name) is not None
    assert lib.anofox_hip_sample_test_record_len() == 12
    pkg = import_pkg()
    for name in ("t_test", "paired_t_test", "yuen", "one_way_anova", "brown_forsythe", "brunner_munzel"):
        for full in (name, name + "_agg"):
            assert pkg.SQL_FUNCTIONS[full] is pkg.SQL_FUNCTIONS["anofox_stats_" + full] is getattr(pkg, full) and full in pkg.__all__
    for name in ("sample_test_batch_host", "sample_test_batch_device", "sample_test_hooks", "parse_sample_test_options"):
        assert callable(getattr(pkg, name)) and name in pkg.__all__
    assert callable(pkg.Context.sample_test_batch_host) and callable(pkg.Context.sample_test_batch_device)


def test_header_compiles_as_c_and_layouts_match_reference_abi():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "anofox_stats_hip.h"
#define O(T, f) printf("%zu ", offsetof(T, f))
int main(void) {
  printf("%zu %zu %zu %zu\n", sizeof(AnofoxAnovaResult), sizeof(AnofoxTTestOptions), sizeof(AnofoxBrunnerMunzelOptions),
         sizeof(AnofoxHipSampleTestBatchOptions));
  O(AnofoxAnovaResult, f_statistic); O(AnofoxAnovaResult, p_value); O(AnofoxAnovaResult, df_between); O(AnofoxAnovaResult, df_within);
  O(AnofoxAnovaResult, ss_between); O(AnofoxAnovaResult, ss_within); O(AnofoxAnovaResult, n_groups); O(AnofoxAnovaResult, n);
  O(AnofoxAnovaResult, method);
  printf("\n");
  O(AnofoxTTestOptions, alternative); O(AnofoxTTestOptions, confidence_level); O(AnofoxTTestOptions, var_equal); O(AnofoxTTestOptions, mu);
  O(AnofoxBrunnerMunzelOptions, alternative); O(AnofoxBrunnerMunzelOptions, confidence_level);
  printf("\n");
  O(AnofoxHipSampleTestBatchOptions, test); O(AnofoxHipSampleTestBatchOptions, alternative); O(AnofoxHipSampleTestBatchOptions, kind);
  O(AnofoxHipSampleTestBatchOptions, mu); O(AnofoxHipSampleTestBatchOptions, trim); O(AnofoxHipSampleTestBatchOptions, confidence_level);
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
    # the layouts of src/include/anofox_stats_ffi.h:1588-1607, 1682-1691, 1799-1804 under gcc, x86-64 SysV
    assert [int(v) for v in out[0].split()] == [72, 32, 16, 40]
    assert [int(v) for v in out[1].split()] == list(range(0, 72, 8))
    assert [int(v) for v in out[2].split()] == [0, 8, 16, 24, 0, 8]
    assert [int(v) for v in out[3].split()] == [0, 4, 8, 16, 24, 32]
    abi = import_pkg("_abi")
    types = (abi.AnofoxAnovaResult, abi.AnofoxTTestOptions, abi.AnofoxBrunnerMunzelOptions, abi.AnofoxHipSampleTestBatchOptions)
    assert [C.sizeof(t) for t in types] == [72, 32, 16, 40]
    offsets = [[getattr(t, f).offset for f, _ in t._fields_] for t in types]
    assert offsets == [list(range(0, 72, 8)), [0, 8, 16, 24], [0, 8], [0, 4, 8, 16, 24, 32]]


def test_option_spellings():
    pkg = import_pkg()
    P = pkg.parse_sample_test_options
    d = P(None)
    assert (d.alternative, d.kind, d.mu, d.trim, d.confidence_level) == (0, 0, 0.0, 0.2, 0.95)
    for name, code in (("two_sided", 0), ("Two-Sided", 0), ("two.sided", 0), ("LESS", 1), ("greater", 2)):
        assert P({"alternative": name}).alternative == code and P({"ALTERNATIVE": name}).alternative == code
    for name, code in (("welch", 0), ("Student", 1), ("PAIRED", 2)):
        assert P({"kind": name}).kind == code and P({"Kind": name}).kind == code
    for name, code in (("fisher", 0), ("Welch", 1)):
        assert P({"kind": name}, 2).kind == code
    assert P({"var_equal": True}).kind == 1 and P({"var_equal": "false"}).kind == 0 and P({"VAR_EQUAL": "true"}).kind == 1
    o = P({"mu": 0.5, "trim": 0.1, "confidence_level": 0.9, "something_else": 3, "alternative": "less", "kind": "student"})
    b = o.batch_options(0)
    assert (b.test, b.alternative, b.kind, b.mu, b.trim, b.confidence_level) == (0, 1, 1, 0.5, 0.1, 0.9)
    assert np.isnan(P({"confidence_level": None}).batch_options(4).confidence_level)
    assert o.method(0) == "Student t-test" and P(None).method(0) == "Welch t-test" and P(None).method(1) == "Yuen test (trim=0.20)"
    assert P(None).method(2) == "Fisher One-way ANOVA" and P(None).method(3) == "Brown-Forsythe test" and P(None).method(4) == "Brunner-Munzel test"
    with pytest.raises(pkg.InvalidInputException, match=r"Unknown alternative 'sideways'"):
        P({"alternative": "sideways"})
    with pytest.raises(pkg.InvalidInputException, match=r"Unknown kind 'paired'"):
        P({"kind": "paired"}, 2)
    with pytest.raises(pkg.InvalidInputException, match=r"Unknown kind 'fisher'"):
        P({"kind": "fisher"})


def _batch(lib, abi, n_groups=1, n_rows=4, off=(0, 4), v=True, y=True, sample=True, records=True, offsets=True, options=GOOD):
    o = np.array(off, np.int64)
    vv, yv, sv, rec = np.ones(64), np.ones(64), np.zeros(64, np.int32), np.zeros(64)
    err = abi.AnofoxError()
    p = lambda a, on: a.ctypes.data_as(_DP) if on else None   # noqa: E731
    ok = lib.anofox_hip_sample_test_batch_host(None, n_groups, n_rows, o.ctypes.data_as(_IP) if offsets else None, p(vv, v), p(yv, y),
                                               sv.ctypes.data_as(_SP) if sample else None, abi.AnofoxHipSampleTestBatchOptions(*options),
                                               p(rec, records), C.byref(err))
    return ok, err.code, err.text()


def _with(**kw):
    names = ("test", "alternative", "kind", "mu", "trim", "confidence_level")
    return tuple(kw.get(n, d) for n, d in zip(names, GOOD))


@pytest.mark.parametrize("kw, text", [
    (dict(v=False), "sample test: row_offsets, v or records is NULL"), (dict(records=False), "sample test: row_offsets, v or records is NULL"),
    (dict(offsets=False), "sample test: row_offsets, v or records is NULL"),
    (dict(y=False, options=_with(kind=2)), "sample test: the paired t-test needs the y column"),
    (dict(sample=False), "sample test: every test but the paired t-test needs the sample column"),
    (dict(sample=False, options=_with(test=3)), "sample test: every test but the paired t-test needs the sample column"),
    (dict(off=(0, 3, 2), n_groups=2), "non-decreasing"), (dict(off=(0, 5)), "non-decreasing"), (dict(off=(-1, 4)), "non-decreasing"),
    (dict(n_groups=-1), "negative"), (dict(n_rows=-1), "negative"),
    (dict(options=_with(test=5)), "sample test: unknown test"), (dict(options=_with(test=-1)), "sample test: unknown test"),
    (dict(options=_with(alternative=3)), "sample test: unknown alternative"), (dict(options=_with(alternative=-1)), "sample test: unknown alternative"),
    (dict(options=_with(kind=3)), "sample test: unknown kind"), (dict(options=_with(test=2, kind=2)), "sample test: unknown kind"),
    (dict(options=_with(test=1, kind=1)), "sample test: unknown kind"), (dict(options=_with(test=4, kind=-1)), "sample test: unknown kind"),
    (dict(options=_with(mu=NAN)), "sample test: mu must be finite"), (dict(options=_with(mu=float("inf"))), "sample test: mu must be finite"),
    (dict(options=_with(test=1, mu=0.5)), "sample test: only the t-test takes a mu"),
    (dict(options=_with(test=2, mu=-1.0)), "sample test: only the t-test takes a mu"),
    (dict(options=_with(test=1, trim=0.5)), "sample test: trim must lie in [0, 0.5)"), (dict(options=_with(trim=-0.1)), "sample test: trim must lie"),
    (dict(options=_with(trim=NAN)), "sample test: trim must lie"),
    (dict(options=_with(confidence_level=0.0)), "sample test: confidence_level must lie in (0, 1)"),
    (dict(options=_with(confidence_level=1.0)), "sample test: confidence_level must lie in (0, 1)")])
def test_batch_argument_errors_come_before_any_device(kw, text):
    abi = import_pkg("_abi")
    ok, code, msg = _batch(abi.load(), abi, **kw)
    assert not ok and code == 1 and text in msg, msg


def test_device_form_checks_its_arguments_first_and_an_empty_call_succeeds():
    abi = import_pkg("_abi")
    lib, err = abi.load(), abi.AnofoxError()
    good, bad = abi.AnofoxHipSampleTestBatchOptions(*GOOD), abi.AnofoxHipSampleTestBatchOptions(*_with(test=9))
    assert not lib.anofox_hip_sample_test_batch_device(None, 1, 4, None, None, None, None, good, None, C.byref(err)) and err.code == 1
    assert not lib.anofox_hip_sample_test_batch_device(None, 1, 4, 8, 8, 8, 8, bad, 8, C.byref(err)) and "sample test: unknown test" in err.text()
    assert not lib.anofox_hip_sample_test_batch_device(None, 1, 4, 8, 8, None, None, good, 8, C.byref(err)) and "sample column" in err.text()
    assert not lib.anofox_hip_sample_test_batch_device(None, 1, 4, 8, 8, None, 8, good, 8, C.byref(err)) and "context is NULL" in err.text()
    assert lib.anofox_hip_sample_test_batch_host(None, 0, 0, None, None, None, None, good, None, C.byref(err)) and err.code == 0   # nothing to do
    nan_level = abi.AnofoxHipSampleTestBatchOptions(*_with(confidence_level=NAN))      # NaN: no interval, not an error
    assert lib.anofox_hip_sample_test_batch_host(None, 0, 0, None, None, None, None, nan_level, None, C.byref(err)) and err.code == 0
    lib.anofox_hip_sample_test_hooks(128)
    lib.anofox_hip_sample_test_hooks(0)


def _array(abi, values):
    a = np.asarray(values, np.float64)
    return abi.AnofoxDataArray(a.ctypes.data_as(_DP), None, len(a)), a


def _scalar(abi, symbol, a, b, options, result):
    res, err = result(), abi.AnofoxError()
    C.memset(C.byref(res), 0xAB, C.sizeof(res))
    (aa, k0), (ba, k1) = _array(abi, a), _array(abi, b)
    return getattr(abi.load(), symbol)(aa, ba, *options, C.byref(res), C.byref(err)), res, err


def test_scalar_failures_leave_the_result_zeroed():
    abi = import_pkg("_abi")
    tt = lambda alt=0, level=0.95, mu=0.0: (abi.AnofoxTTestOptions(alt, level, False, mu),)   # noqa: E731
    bm = lambda alt=0, level=0.95: (abi.AnofoxBrunnerMunzelOptions(alt, level),)              # noqa: E731
    T, A = abi.AnofoxTestResult, abi.AnofoxAnovaResult
    cases = [("anofox_t_test", [1.0], [1.0, 2.0], tt(), T, "t-test requires at least 2 observations in group 1"),
             ("anofox_t_test", [1.0, 2.0], [NAN, 2.0], tt(), T, "t-test requires at least 2 observations in group 2"),
             ("anofox_t_test", [1.0, 2.0], [3.0, 4.0], tt(alt=7), T, "sample test: unknown alternative"),
             ("anofox_t_test", [1.0, 2.0], [3.0, 4.0], tt(mu=float("inf")), T, "sample test: mu must be finite"),
             ("anofox_t_test", [1.0, 2.0], [3.0, 4.0], tt(level=1.5), T, "sample test: confidence_level must lie in (0, 1)"),
             ("anofox_yuen_test", [1.0, 2.0, 3.0], [1.0, 2.0, 3.0, 4.0], (0.2, 0, 0.95), T, "Yuen test requires at least 4 observations in group 1"),
             ("anofox_yuen_test", [1.0, 2.0, 3.0, 4.0], [1.0, 2.0, 3.0], (0.2, 0, 0.95), T, "Yuen test requires at least 4 observations in group 2"),
             ("anofox_yuen_test", [1.0, 2.0, 3.0, 4.0], [1.0, 2.0, 3.0, 5.0], (0.5, 0, 0.95), T, "sample test: trim must lie in [0, 0.5)"),
             ("anofox_brunner_munzel", [1.0], [1.0, 2.0], bm(), T, "Brunner-Munzel test requires at least 2 observations in group 1"),
             ("anofox_brunner_munzel", [1.0, 3.0], [NAN], bm(), T, "Brunner-Munzel test requires at least 2 observations in group 2"),
             ("anofox_brunner_munzel", [1.0, 3.0], [2.0, 4.0], bm(alt=-1), T, "sample test: unknown alternative"),
             ("anofox_one_way_anova", [1.0, 2.0, 3.0, 4.0], [0.0, 0.0, 0.9, -0.9], (), A, "ANOVA requires at least 2 groups"),
             ("anofox_one_way_anova", [1.0, 2.0, 3.0, NAN], [5.0, 5.0, 7.0, 7.0], (), A,
              "ANOVA requires at least 2 observations per group (group 1 has 1)"),
             ("anofox_brown_forsythe", [1.0, 2.0, 3.0], [2.0, 2.0, 2.0], (), T, "Brown-Forsythe test requires at least 2 groups"),
             ("anofox_brown_forsythe", [1.0, 2.0, 3.0], [2.0, 1.0, 1.0], (), T,
              "Brown-Forsythe test requires at least 2 observations per group (group 0 has 1)")]
    for symbol, a, b, options, result, text in cases:
        ok, res, err = _scalar(abi, symbol, a, b, options, result)
        assert not ok and err.code == 1 and text in err.text(), err.text()
        assert bytes(res) == bytes(C.sizeof(res))          # every field 0, the pointer NULL: nothing to free
        getattr(abi.load(), "anofox_free_anova_result" if result is A else "anofox_free_test_result")(C.byref(res))   # harmless
    err, empty = abi.AnofoxError(), abi.AnofoxDataArray(None, None, 0)
    assert not abi.load().anofox_t_test(empty, empty, *tt(), None, C.byref(err)) and "out_result is NULL" in err.text()
    assert not abi.load().anofox_one_way_anova(empty, empty, None, C.byref(err)) and "out_result is NULL" in err.text()
    assert not abi.load().anofox_brown_forsythe(empty, empty, None, C.byref(err)) and "out_result is NULL" in err.text()


def test_python_refuses_bad_input_before_any_device():
    pkg = import_pkg()
    with pytest.raises(pkg.InvalidInputException, match="paired t-test takes two value columns"):
        pkg.t_test([1.0, 2.0], [3.0, 4.0], {"kind": "paired"})
    with pytest.raises(pkg.InvalidInputException, match="requires equal length samples"):
        pkg.paired_t_test([1.0, 2.0, 3.0], [3.0, 4.5])
    with pytest.raises(pkg.InvalidInputException, match="same number of rows"):
        pkg.t_test_agg(["a", "a"], [1.0, 2.0], [0])
    with pytest.raises(pkg.InvalidInputException, match="at least 4 observations in group 1"):
        pkg.yuen([1.0, 2.0], [3.0, 4.0, 5.0, 6.0])
    with pytest.raises(pkg.AnofoxStatsError, match="trim must lie"):
        pkg.yuen_agg(["a"] * 4, [1.0, 2.0, 3.0, 4.0], [0, 0, 1, 1], {"trim": 0.7})
