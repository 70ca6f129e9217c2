"""CPU-side checks of the correlation surface: the header compiles as C, the struct layouts (the reference's ABI), the exported
symbols, the option spellings, and the argument errors that are answered before any GPU work."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT, import_pkg

COR_SYMBOLS = ("anofox_hip_cor_record_len", "anofox_hip_cor_batch_device", "anofox_hip_cor_batch_host", "anofox_hip_cor_test_hooks",
               "anofox_pearson_cor", "anofox_spearman_cor", "anofox_kendall_cor", "anofox_free_correlation_result")
_DP = C.POINTER(C.c_double)
_IP = C.POINTER(C.c_int64)
NAN = float("nan")


def test_symbols_present():
    abi = import_pkg("_abi")
    lib = abi.load()
    for name in COR_SYMBOLS:
        assert name in abi.SYMBOLS and getattr(lib, name) is not None
    assert lib.anofox_hip_cor_record_len() == 8
    pkg = import_pkg()
    for name in ("pearson", "spearman", "kendall", "pearson_agg", "spearman_agg", "kendall_agg"):
        assert pkg.SQL_FUNCTIONS[name] is pkg.SQL_FUNCTIONS["anofox_stats_" + name] is getattr(pkg, name) and name in pkg.__all__
    for name in ("cor_batch_host", "cor_batch_device", "cor_test_hooks"):
        assert callable(getattr(pkg, name)) and name in pkg.__all__
    assert callable(pkg.Context.cor_batch_host) and callable(pkg.Context.cor_batch_device)


def test_header_compiles_as_c_and_layouts_match_reference_abi():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "anofox_stats_hip.h"
#define O(T, f) printf("%zu ", offsetof(T, f))
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(AnofoxCorrelationOptions), sizeof(AnofoxKendallOptions), sizeof(AnofoxCorrelationResult),
         sizeof(AnofoxHipCorBatchOptions), sizeof(AnofoxAlternative), sizeof(AnofoxKendallType));
  O(AnofoxCorrelationOptions, alternative); O(AnofoxCorrelationOptions, confidence_level);
  O(AnofoxKendallOptions, alternative); O(AnofoxKendallOptions, tau_type); O(AnofoxKendallOptions, confidence_level);
  O(AnofoxCorrelationResult, r); O(AnofoxCorrelationResult, statistic); O(AnofoxCorrelationResult, p_value);
  O(AnofoxCorrelationResult, ci_lower); O(AnofoxCorrelationResult, ci_upper); O(AnofoxCorrelationResult, confidence_level);
  O(AnofoxCorrelationResult, n); O(AnofoxCorrelationResult, method);
  O(AnofoxHipCorBatchOptions, method); O(AnofoxHipCorBatchOptions, alternative); O(AnofoxHipCorBatchOptions, tau_type);
  O(AnofoxHipCorBatchOptions, confidence_level);
  printf("\n%d %d %d %d %d %d\n", ANOFOX_ALTERNATIVE_TWO_SIDED, ANOFOX_ALTERNATIVE_LESS, ANOFOX_ALTERNATIVE_GREATER,
         ANOFOX_KENDALL_TAU_A, ANOFOX_KENDALL_TAU_B, ANOFOX_KENDALL_TAU_C);
  return 0;
}
'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.check_output([exe]).decode().split("\n")
    # the layouts of src/include/anofox_stats_ffi.h:1611-1628, 1709-1738 under gcc, x86-64 SysV
    assert [int(v) for v in out[0].split()] == [16, 16, 64, 24, 4, 4]
    assert [int(v) for v in out[1].split()] == [0, 8, 0, 4, 8, 0, 8, 16, 24, 32, 40, 48, 56, 0, 4, 8, 16]
    assert [int(v) for v in out[2].split()] == [0, 1, 2, 0, 1, 2]
    abi = import_pkg("_abi")
    assert [C.sizeof(t) for t in (abi.AnofoxCorrelationOptions, abi.AnofoxKendallOptions, abi.AnofoxCorrelationResult,
                                  abi.AnofoxHipCorBatchOptions)] == [16, 16, 64, 24]
    assert [getattr(abi.AnofoxCorrelationResult, f).offset for f, _ in abi.AnofoxCorrelationResult._fields_] == list(range(0, 64, 8))
    assert [getattr(abi.AnofoxHipCorBatchOptions, f).offset for f, _ in abi.AnofoxHipCorBatchOptions._fields_] == [0, 4, 8, 16]
    assert abi.AnofoxKendallOptions.tau_type.offset == 4 and abi.AnofoxKendallOptions.confidence_level.offset == 8


def test_option_spellings():
    pkg = import_pkg()
    P = pkg.parse_correlation_options
    d = P(None)
    assert (d.alternative, d.tau_type, d.confidence_level) == (0, 1, 0.95)
    for name, code in (("two_sided", 0), ("Two-Sided", 0), ("two.sided", 0), ("LESS", 1), ("greater", 2)):
        assert P({"alternative": name}).alternative == code and P({"ALTERNATIVE": name}).alternative == code
    for name, code in (("a", 0), ("B", 1), ("c", 2), ("tau_a", 0), ("TauC", 2)):
        assert P({"tau_type": name}).tau_type == code and P({"Variant": name}).tau_type == code
    assert P({"confidence_level": 0.99, "something_else": 3}).confidence_level == 0.99
    o = P({"tau_type": "c", "alternative": "less", "confidence_level": 0.9})
    b, k = o.batch_options(2), o.kendall_ffi_options()
    assert (b.method, b.alternative, b.tau_type, b.confidence_level) == (2, 1, 2, 0.9) and (k.alternative, k.tau_type) == (1, 2)
    assert o.method_text(2) == "Kendall's TauC" and o.method_text(0) == "Pearson correlation" and o.method_text(1) == "Spearman rank correlation"
    with pytest.raises(pkg.InvalidInputException, match=r"Unknown alternative 'sideways'"):
        P({"alternative": "sideways"})
    with pytest.raises(pkg.InvalidInputException, match=r"Unknown tau_type 'd'"):
        P({"tau_type": "d"})


def _batch(lib, abi, n_groups=1, n_rows=4, off=(0, 4), x=True, y=True, records=True, offsets=True, options=(0, 0, 1, 0.95)):
    o = np.array(off, np.int64)
    xv, yv, rec = np.ones(64), np.ones(64), np.zeros(64)
    err = abi.AnofoxError()
    p = lambda a, on: a.ctypes.data_as(_DP) if on else None   # noqa: E731
    ok = lib.anofox_hip_cor_batch_host(None, n_groups, n_rows, o.ctypes.data_as(_IP) if offsets else None, p(xv, x), p(yv, y),
                                       abi.AnofoxHipCorBatchOptions(*options), p(rec, records), C.byref(err))
    return ok, err.code, err.text()


@pytest.mark.parametrize("kw, text", [
    (dict(x=False), "x column pointer is NULL"), (dict(y=False), "correlation: row_offsets, y or records is NULL"),
    (dict(records=False), "correlation: row_offsets, y or records is NULL"), (dict(offsets=False), "correlation: row_offsets, y or records is NULL"),
    (dict(off=(0, 3, 2), n_groups=2), "non-decreasing"), (dict(off=(0, 5)), "non-decreasing"), (dict(off=(-1, 4)), "non-decreasing"),
    (dict(n_groups=-1), "negative"), (dict(n_rows=-1), "negative"),
    (dict(options=(3, 0, 1, 0.95)), "correlation: unknown method"), (dict(options=(-1, 0, 1, 0.95)), "correlation: unknown method"),
    (dict(options=(0, 3, 1, 0.95)), "correlation: unknown alternative"), (dict(options=(2, 0, 3, 0.95)), "correlation: unknown tau_type"),
    (dict(options=(0, 0, 1, 0.0)), "correlation: confidence_level must lie in (0, 1)"),
    (dict(options=(1, 0, 1, 1.0)), "correlation: confidence_level must lie in (0, 1)"),
    (dict(options=(0, 0, 1, float("inf"))), "correlation: confidence_level must lie in (0, 1)")])
def test_batch_argument_errors_come_before_any_device(kw, text):
    abi = import_pkg("_abi")
    ok, code, msg = _batch(abi.load(), abi, **kw)
    assert not ok and code == 1 and text in msg, msg


def test_device_form_checks_its_arguments_first_and_an_empty_call_succeeds():
    abi = import_pkg("_abi")
    lib, err = abi.load(), abi.AnofoxError()
    good, bad = abi.AnofoxHipCorBatchOptions(0, 0, 1, NAN), abi.AnofoxHipCorBatchOptions(5, 0, 1, 0.95)
    assert not lib.anofox_hip_cor_batch_device(None, 1, 4, None, None, None, good, None, C.byref(err)) and err.code == 1
    assert not lib.anofox_hip_cor_batch_device(None, 1, 4, 8, 8, 8, bad, 8, C.byref(err)) and "correlation: unknown method" in err.text()
    assert not lib.anofox_hip_cor_batch_device(None, 1, 4, 8, 8, 8, good, 8, C.byref(err)) and "context is NULL" in err.text()
    assert lib.anofox_hip_cor_batch_host(None, 0, 0, None, None, None, good, None, C.byref(err)) and err.code == 0   # nothing to do
    lib.anofox_hip_cor_test_hooks(128)
    lib.anofox_hip_cor_test_hooks(0)


def _scalar(abi, symbol, x, y, options):
    xv, yv = np.asarray(x, np.float64), np.asarray(y, np.float64)
    res, err = abi.AnofoxCorrelationResult(), abi.AnofoxError()
    C.memset(C.byref(res), 0xAB, C.sizeof(res))
    ok = getattr(abi.load(), symbol)(abi.AnofoxDataArray(xv.ctypes.data_as(_DP), None, len(xv)),
                                     abi.AnofoxDataArray(yv.ctypes.data_as(_DP), None, len(yv)), options, C.byref(res), C.byref(err))
    return ok, res, err


@pytest.mark.parametrize("symbol, name", [("anofox_pearson_cor", "Pearson"), ("anofox_spearman_cor", "Spearman"), ("anofox_kendall_cor", "Kendall")])
def test_scalar_failures_leave_the_result_zeroed(symbol, name):
    abi = import_pkg("_abi")
    make = (lambda alt=0, level=0.95, tau=1: abi.AnofoxKendallOptions(alt, tau, level)) if name == "Kendall" else \
        (lambda alt=0, level=0.95, tau=1: abi.AnofoxCorrelationOptions(alt, level))
    cases = [([1.0, 2.0, 3.0], [1.0, 2.0], make(), name + " correlation requires equal length vectors"),
             ([1.0, 2.0], [1.0, 2.0], make(), name + " correlation requires at least 3 valid pairs"),
             ([1.0, 2.0, NAN, 4.0], [1.0, NAN, 3.0, 4.0], make(), name + " correlation requires at least 3 valid pairs"),
             ([1.0, 2.0, 3.0], [1.0, 2.0, 4.0], make(alt=7), "correlation: unknown alternative")]
    if name == "Kendall":
        cases.append(([1.0, 2.0, 3.0], [1.0, 2.0, 4.0], make(tau=9), "correlation: unknown tau_type"))
    else:
        cases.append(([1.0, 2.0, 3.0], [1.0, 2.0, 4.0], make(level=1.5), "correlation: confidence_level must lie in (0, 1)"))
    for x, y, options, text in cases:
        ok, res, err = _scalar(abi, symbol, x, y, options)
        assert not ok and err.code == 1 and text in err.text(), err.text()
        assert bytes(res) == bytes(C.sizeof(res))                 # every field 0, the pointer NULL: nothing to free
        abi.load().anofox_free_correlation_result(C.byref(res))   # and freeing it is harmless
    err = abi.AnofoxError()
    empty = abi.AnofoxDataArray(None, None, 0)
    assert not getattr(abi.load(), symbol)(empty, empty, make(), None, C.byref(err)) and "out_result is NULL" in err.text()
